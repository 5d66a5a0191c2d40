"""Operands, float64 references and bars of the split-bf16 ("x3", MMAD_BF16X3)
GEMM tests: tests/test_x3_reference.py checks them against each other on the
CPU, tests/test_gpu_x3_matrix.py checks the kernel against them.  Plain torch
on the host, nothing from the library.

An fp32 operand v travels as hi = RNE_bf16(v), lo = RNE_bf16(v - hi).  Two
references of y = affine(act(x . w^T + bias)), both float64:

  P3  from Ah.Bh^T + Ah.Bl^T + Al.Bh^T of the planes: what the kernel is
      defined to compute.  fp32-valued outputs (diff, rowsq, NAP score) hold
      |got - ref| <= 2e-5 max|ref| (the project's fp32 bar: the kernel shares
      fp32 accumulation with the fp32 path); a value read back from the stored
      planes, hi + lo, may be off by another 2^-17 |ref| (hi has 8 significand
      bits, so the residual is at most 2^-8 of the value's binade and lo
      rounds it by at most half an ulp of that, 2^-17).
  T   the true product of the fp32 operands.  |got - ref| <= 3 * 2^-18 D +
      2e-5 max|ref| with D = |x| . |w|^T + |bias|, carried through the affine
      as D |scale| + |shift|; every activation is 1-Lipschitz, so D bounds
      them too.  The 3: the two operands' representation and the dropped
      lo . lo term (test_gpu_x3.py's bar with the measured fp32 error replaced
      by the fp32 bar).  Values read back from the planes get the same
      2^-17 |ref| as above."""
import torch

ACT_NONE, ACT_LEAKY, ACT_RELU, ACT_SIGMOID, ACT_TANH = range(5)
ACT_NAME = {ACT_NONE: "none", ACT_LEAKY: "leaky", ACT_RELU: "relu", ACT_SIGMOID: "sigmoid",
            ACT_TANH: "tanh"}
SLOPE = 0.2
FP32_BAR = 2e-5
T_REL = 3 * 2.0 ** -18
PLANE_REL = 2.0 ** -17


def planes_of(v):
    hi = v.bfloat16()
    return hi, (v - hi.float()).bfloat16()


def pad(n, g=128):
    return (int(n) + g - 1) // g * g


def act64(z, act):
    slope = float(torch.tensor(SLOPE, dtype=torch.float32))      # the float the kernel gets
    if act == ACT_LEAKY:
        return torch.where(z > 0, z, z * slope)
    if act == ACT_RELU:
        return z.clamp_min(0.0)
    if act == ACT_SIGMOID:
        return torch.sigmoid(z)
    if act == ACT_TANH:
        return torch.tanh(z)
    return z


class Problem:
    """One masked GEMM problem: fp32 operands (randn; the weights scaled by
    0.05 as in test_gpu_gemm_matrix.py), zero on padding, their planes, and
    the float64 references.  Everything lives on the CPU and is read only."""

    def __init__(self, M, N, K, Mp=None, Np=None, Kp=None, seed=0):
        Mp, Np, Kp = Mp or pad(M), Np or pad(N), Kp or pad(K)
        self.dims = (M, N, K, Mp, Np, Kp)
        g = torch.Generator().manual_seed(20270 + seed)

        def mat(rows, cols, prows, pcols, scale=1.0):
            t = torch.zeros(prows, pcols)
            t[:rows, :cols] = torch.randn(rows, cols, generator=g) * scale
            return t

        def vec(n, scale, shift=0.0):
            t = torch.zeros(Np)
            t[:n] = torch.randn(n, generator=g) * scale + shift
            return t
        self.x = mat(M, K, Mp, Kp)
        self.w = mat(N, K, Np, Kp, 0.05)
        self.b = vec(N, 0.1)
        self.sc = vec(N, 0.1, 1.0)                 # eval-BN affine, 0 on padding
        self.sh = vec(N, 0.1)
        self.colw = torch.zeros(Np)                # NAP column weights in [0.5, 1.5]
        self.colw[:N] = torch.rand(N, generator=g) + 0.5
        # the score reference: fp32 [Mp][Np], NaN on padding (only the valid region may be read)
        self.ref = torch.full((Mp, Np), float("nan"))
        self.ref[:M, :N] = torch.randn(M, N, generator=g)
        self.xp = torch.stack(planes_of(self.x))   # [2][Mp][Kp] bf16
        self.wp = torch.stack(planes_of(self.w))   # [2][Np][Kp] bf16
        xh, xl = (t[:M, :K].double() for t in self.xp)
        wh, wl = (t[:N, :K].double() for t in self.wp)
        xd, wd, bd = self.x[:M, :K].double(), self.w[:N, :K].double(), self.b[:N].double()
        self.z_p3 = xh @ wh.t() + (xh @ wl.t() + xl @ wh.t()) + bd
        self.z_hh = xh @ wh.t() + bd               # the single-plane (plain bf16) product
        self.z_t = xd @ wd.t() + bd
        self.d = xd.abs() @ wd.abs().t() + bd.abs()
        self._y = {}

    def y(self, which, act, affine):
        """float64 [M][N]; which: "p3", "t" or "hh"."""
        key = (which, act, affine)
        if key not in self._y:
            N = self.dims[1]
            a = act64(getattr(self, "z_" + which), act)
            if affine:
                a = a * self.sc[:N].double() + self.sh[:N].double()
            self._y[key] = a
        return self._y[key]

    def dy(self, affine):
        """D carried through the affine."""
        N = self.dims[1]
        return self.d * self.sc[:N].double().abs() + self.sh[:N].double().abs() if affine else self.d


def p3_bound(ref, stored):
    """elementwise bound of an output against the P3 reference"""
    b = FP32_BAR * ref.abs().max() + 1e-300
    return b + PLANE_REL * ref.abs() if stored else b + torch.zeros_like(ref)


def t_bound(ref, dy, stored):
    """elementwise bound of an output against the true-product reference"""
    b = T_REL * dy + FP32_BAR * ref.abs().max()
    return b + PLANE_REL * ref.abs() if stored else b


# the problems of the matrix (section "one masked problem"): the ragged 512^3
# problem of test_gpu_gemm_matrix.py (a 4 x 4 grid, a partial last row tile,
# column 300 inside a lane's 4-column quad, the column group 384..511 fully
# masked) and the smallest the kernel takes: one tile, two K stages, one row.
MAIN = dict(M=400, N=300, K=489, Mp=512, Np=512, Kp=512, seed=1)
MINI = dict(M=1, N=3, K=1, Mp=128, Np=128, Kp=128, seed=2)
_CACHE = {}


def problem(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _CACHE:
        _CACHE[key] = Problem(**kw)
    return _CACHE[key]
