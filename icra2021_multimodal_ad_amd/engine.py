"""NativeAE: owner of the device buffers of one autoencoder and the handle of
the native executor (``mmad_ae_*`` in include/mmad.h).

Memory layout (DESIGN.md "Data layout in HBM"): one flat fp32 parameter
buffer (all weights [Np][Kp] first, then per-layer bias/gamma/beta, every
dimension zero-padded to 128), same-shaped flat grads and Adam m/v, a bf16
shadow of the weight region for the bf16 path, and a [2][n_bn] running-stat
buffer.  The reference-shaped ``nn.Parameter``s of the plugin surface are
strided views into these buffers, so ``state_dict`` / ``load_state_dict`` /
``torch.optim`` all see the same memory the kernels use.
"""
import ctypes

import torch

from . import _native
from ._native import call, ptr, stream_ptr

DTYPES = {"f32": _native.F32, "fp32": _native.F32, "float32": _native.F32,
          "bf16": _native.BF16, "bfloat16": _native.BF16}


class NativeAE:
    def __init__(self, enc_widths, dec_widths, vib=False, dtype="bf16", device=None,
                 slope=0.2, bn_eps=1e-5, bn_momentum=0.1):
        lib = _native.load()
        self.dtype_name = "bf16" if DTYPES[dtype] == _native.BF16 else "f32"
        self.dt = DTYPES[dtype]
        self.enc_widths = [int(w) for w in enc_widths]
        self.dec_widths = [int(w) for w in dec_widths]
        self.vib = bool(vib)
        self.n_enc, self.n_dec = len(enc_widths) - 1, len(dec_widths) - 1
        self.btl = self.dec_widths[0]
        self.bn_eps, self.bn_momentum = bn_eps, bn_momentum
        h = ctypes.c_void_p()
        ea = (ctypes.c_int * len(enc_widths))(*self.enc_widths)
        da = (ctypes.c_int * len(dec_widths))(*self.dec_widths)
        call("mmad_ae_create", ctypes.byref(h), self.dt, self.n_enc, ea, self.n_dec, da,
             int(self.vib), float(slope), float(bn_eps), float(bn_momentum))
        self._h = h
        self._lib = lib
        if _native.SCHEDULE["dw_group"] is not None or _native.SCHEDULE["dw_group_members"] is not None:
            # grouped dW launches of the ping-pong step: None = the library's own default
            blocks, members = _native.SCHEDULE["dw_group"], _native.SCHEDULE["dw_group_members"]
            # (the setter leaves a value as it is for blocks < -1 / members <= 0)
            call("mmad_ae_set_dw_group", h, -2 if blocks is None else int(blocks),
                 0 if members is None else int(members))
        n_l = self.n_enc + self.n_dec
        info = (ctypes.c_int64 * (7 * n_l))()
        tot = (ctypes.c_int64 * 4)()
        call("mmad_ae_layout", h, info, tot)
        self.n_params, self.n_weight, self.n_bn = int(tot[0]), int(tot[1]), int(tot[2])
        widths = [(self.enc_widths[i], self.enc_widths[i + 1], True) for i in range(self.n_enc)] + \
                 [(self.dec_widths[i], self.dec_widths[i + 1], False) for i in range(self.n_dec)]
        self.layers = []
        for i, (k, n, enc) in enumerate(widths):
            r = [int(v) for v in info[7 * i: 7 * i + 7]]
            self.layers.append(dict(K=k, N=n, enc=enc, w_off=r[0], b_off=r[1], g_off=r[2],
                                    be_off=r[3], Kp=r[4], Np=r[5], bn_off=r[6], bn=r[2] >= 0))
        device = torch.device(device) if device is not None else torch.device("cpu")
        self.device = device
        self._alloc(device)
        self._ws = None
        self._synced_version = None
        self._score_precision = None   # set_score_precision: None or "bf16x3"
        self._planes = None
        self._nap = None               # set_nap: the attached fit's tensors (kept alive here)
        # version of the fp32 master as the plugin surface sees it: the
        # reference-shaped nn.Parameters are views with their OWN version
        # counters (load_state_dict / a torch optimizer bump those, not
        # params._version), so the owner installs a callable summing them
        self.version_fn = None
        # bumped by every native call that rewrites the workspace; a
        # differentiable forward records it and its backward checks it
        self.gen = 0
        self.adam_step_count = 0
        self.use_graph = bool(_native.SCHEDULE["train_graph"])

    # ------------------------------------------------------------------ memory
    def _alloc(self, device, src=None):
        kw = dict(device=device, dtype=torch.float32)
        self.params = torch.zeros(self.n_params, **kw)
        self.grads = torch.zeros(self.n_params, **kw)
        self.exp_avg = torch.zeros(self.n_params, **kw)
        self.exp_avg_sq = torch.zeros(self.n_params, **kw)
        # (one element for a model without BatchNorm -- a one-layer encoder and
        # decoder: the native handle takes a null running pointer for unbound)
        self.running = torch.zeros(max(2 * self.n_bn, 1), **kw)
        self.running[self.n_bn:] = 1.0
        # bf16: two weight shadows (mmad_ae_set_shadow_pair), ping-ponged by
        # the fused step on large calls (the executor picks per call: knob
        # pair_rows); _native.SCHEDULE["shadow_pair"] = False keeps one
        self._pair = self.dt == _native.BF16 and bool(_native.SCHEDULE["shadow_pair"])
        self._shadow_buf = (torch.zeros((2 if self._pair else 1) * self.n_weight, device=device,
                                        dtype=torch.bfloat16)
                            if self.dt == _native.BF16 else None)
        if src is not None:
            for name in ("params", "grads", "exp_avg", "exp_avg_sq", "running"):
                getattr(self, name).copy_(getattr(src, name))
        self._bind()

    def _bind(self):
        self._synced_version = None
        if self.device.type != "cuda":
            return
        sb = self._shadow_buf
        call("mmad_ae_bind", self._h, ptr(self.params), ptr(self.grads), ptr(self.exp_avg),
             ptr(self.exp_avg_sq), ptr(sb[: self.n_weight] if sb is not None else None),
             ptr(self.running))
        if self._pair:
            call("mmad_ae_set_shadow_pair", self._h, ptr(sb[self.n_weight:]))
        if getattr(self, "_score_precision", None) is not None:
            # the score planes follow the buffers (a rebind, a new device)
            if self._planes is None or self._planes.device != self.device:
                self._planes = torch.zeros(2 * self.n_weight, device=self.device, dtype=torch.bfloat16)
            call("mmad_ae_set_score_planes", self._h, ptr(self._planes))
        if getattr(self, "_nap", None) is not None:
            # a NAP fit lives on one device and names score planes that may be gone
            self._nap = None
            call("mmad_ae_set_nap", self._h, 0, 0, 0, None, None, None, _native.F32, None, None)
        if getattr(self, "_grad_bf16", None) is not None:
            # the bf16 exchange scratch follows the buffers to their new device
            self.set_grad_bf16(True)

    @property
    def shadow(self):
        """The bf16 weight shadow the kernels read next (None for fp32)."""
        sb = self._shadow_buf
        if sb is None:
            return None
        if not self._pair or self.device.type != "cuda":
            return sb[: self.n_weight]
        cur = self._lib.mmad_ae_current_shadow(self._h) or 0
        return sb[self.n_weight:] if cur != sb.data_ptr() else sb[: self.n_weight]

    def to(self, device):
        device = torch.device(device)
        if device == self.device:
            return self
        old = _Snapshot(self)
        self.device = device
        self._alloc(device, src=old)
        self._ws = None
        self._dw_streams = None   # the torch exchange's bucket streams belong to the old device
        return self

    def set_score_precision(self, precision):
        """``"bf16x3"``: an fp32 model's eval forward / validate / score passes
        run their GEMMs on the bf16 matrix cores over split-bf16 weight planes
        (mmad_ae_set_score_planes; this object owns the 2*n_weight bf16
        buffer); training is untouched.  ``None`` detaches."""
        if precision not in (None, "bf16x3"):
            raise ValueError(f"score precision {precision!r}: expected 'bf16x3' or None")
        if precision is not None and self.dt != _native.F32:
            raise ValueError("score precision 'bf16x3' is for fp32 models (a bf16 model scores on "
                             "its own shadow)")
        if self._nap is not None:
            self.set_nap(None)         # an attached fit names the precision it was attached under
        self._score_precision = precision
        self._synced_version = None
        self._ws = None            # the workspace size depends on it
        if precision is None:
            self._planes = None
            if self.device.type == "cuda":
                call("mmad_ae_set_score_planes", self._h, None)
        elif self.device.type == "cuda":
            self._bind()

    def set_nap(self, fit, start=0, end=None, precision="f32"):
        """Attach a NAP fit to the scoring passes (mmad_ae_set_nap): ``fit`` =
        (R, vt [Rp, Kp], bias [Rp], w [Rp]) fp32 on this device, as NapScorer
        lays them out, over the diff layers [start, end); ``precision`` = the
        NAP GEMM's, "f32" (exact) or "bf16x3" (needs
        set_score_precision("bf16x3")).  ``score(..., nap_out=)`` and
        ``score_stream(..., nap_out=)`` then also write the per-window NAP
        scores.  The tensors are read when a pass runs (re-fitting them in
        place is seen; "bf16x3" splits vt once, here).  ``None`` detaches."""
        if fit is None:
            self._nap = None
            if self.device.type == "cuda":
                call("mmad_ae_set_nap", self._h, 0, 0, 0, None, None, None, _native.F32, None, None)
            return
        if precision not in ("f32", "bf16x3"):
            raise ValueError(f"NAP precision {precision!r}: expected 'f32' or 'bf16x3'")
        R, vt, bias, w = fit
        end = self.n_enc + 1 if end is None else int(end)
        for t in (vt, bias, w):
            self._require(t)
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("set_nap: vt / bias / w must be contiguous fp32 tensors")
        W = sum(self.diff_widths()[int(start):end])
        if tuple(vt.shape) != (_native.pad(R), _native.pad(W)) or bias.numel() != vt.shape[0] \
                or w.numel() != vt.shape[0]:
            raise ValueError(f"set_nap: fit shapes {tuple(vt.shape)} do not match R={R}, W={W}")
        x3 = precision == "bf16x3"
        planes = torch.empty((2,) + tuple(vt.shape), device=self.device, dtype=torch.bfloat16) if x3 else None
        call("mmad_ae_set_nap", self._h, int(start), end, int(R), ptr(vt), ptr(bias), ptr(w),
             _native.BF16X3 if x3 else _native.F32, ptr(planes), stream_ptr())
        self._nap = (vt, bias, w, planes)

    def nap_operand(self, B):
        """(byte offset in the aligned workspace, Mp, Kp, W, dtype) of the packed
        NAP operand for a batch of B windows (mmad_ae_nap_operand)."""
        info = (ctypes.c_int64 * 5)()
        call("mmad_ae_nap_operand", self._h, int(B), info)
        return tuple(int(v) for v in info)

    @property
    def score_dtype(self):
        """MMAD dtype of the eval / score GEMMs (F32, BF16 or BF16X3)."""
        return int(self._lib.mmad_ae_score_dtype(self._h))

    def set_comm(self, comm):
        """Attach a dist.NativeComm (or None): mmad_ae_train_step then exchanges
        the weight gradients in buckets of consecutive layers (tune knob
        dp_bucket_mib) on the executor's comm stream before their Adam
        (sharded: reduce-scatter, Adam on this rank's 1/N, all-gather).
        Detaching first all-gathers the sharded master weights / Adam moments
        (sync_master: collective, so detach on every rank at the same point)."""
        if comm is None and getattr(self, "_comm", None) is not None:
            self.sync_master()
        self._comm = comm        # keep the communicator alive as long as the handle uses it
        call("mmad_ae_set_comm", self._h, comm.handle if comm is not None else None)

    def set_grad_bf16(self, on=True):
        """Optional bf16 gradient exchange of the sharded DP buckets
        (mmad_ae_set_grad_bf16): this object owns the bf16 scratch buffer."""
        self._grad_bf16 = (torch.empty(self.n_weight, device=self.device, dtype=torch.bfloat16)
                           if on else None)
        call("mmad_ae_set_grad_bf16", self._h, ptr(self._grad_bf16))

    @property
    def master_stale(self):
        """True while the sharded DP step has left the fp32 master weights (bf16
        model) / the Adam moments current only on their owning rank."""
        return bool(self._lib.mmad_ae_dp_master_stale(self._h))

    def sync_master(self):
        """All-gather the shards of the master weights and Adam moments after
        sharded DP steps (collective: every rank, same point; a no-op when
        nothing is stale)."""
        if self.master_stale:
            call("mmad_ae_dp_sync_master", self._h, stream_ptr())

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None:
                self._lib.mmad_ae_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ---------------------------------------------------------------- views
    def _vec(self, buf, off, n):
        return buf[off: off + n]

    def weight_view(self, buf, l):
        L = self.layers[l]
        return buf[L["w_off"]: L["w_off"] + L["Np"] * L["Kp"]].view(L["Np"], L["Kp"])[:L["N"], :L["K"]]

    def param_views(self, buf, l):
        """Reference-shaped views of layer ``l`` in flat buffer ``buf``:
        (weight[N,K], bias[N], gamma[N] | None, beta[N] | None)."""
        L = self.layers[l]
        w = self.weight_view(buf, l)
        b = self._vec(buf, L["b_off"], L["N"])
        g = self._vec(buf, L["g_off"], L["N"]) if L["bn"] else None
        be = self._vec(buf, L["be_off"], L["N"]) if L["bn"] else None
        return w, b, g, be

    def running_views(self, l):
        L = self.layers[l]
        if not L["bn"]:
            return None, None
        o, n = L["bn_off"], L["N"]
        return self.running[o: o + n], self.running[self.n_bn + o: self.n_bn + o + n]

    # -------------------------------------------------------------- helpers
    def _require(self, x):
        _native.require_gpu(x)
        if self.device.type != "cuda":
            raise _native.NativeUnavailable("model buffers are on the CPU; call .cuda() first")

    def master_version(self):
        return self.version_fn() if self.version_fn is not None else self.params._version

    def sync_shadow(self, force=False):
        """Refresh the bf16 weight shadow if the fp32 master was written by
        anything other than the native Adam (load_state_dict, torch optim);
        for an fp32 model with score planes attached, the planes."""
        if (self.shadow is None and self._planes is None) or self.device.type != "cuda":
            return
        v = self.master_version()
        if force or v != self._synced_version:
            call("mmad_ae_sync_shadow", self._h, stream_ptr())
            self._synced_version = v

    def _mark_synced(self):
        """The native Adam just wrote the master AND the shadow."""
        if self.shadow is not None or self._planes is not None:
            self._synced_version = self.master_version()

    def check_status(self):
        """Raise NativeError if a split-K GEMM combine of the calls since the
        last check timed out (a no-op unless split-K is enabled)."""
        if self._ws is None or self.device.type != "cuda":
            return
        base = self._ws.data_ptr()
        aligned = (base + 255) // 256 * 256
        call("mmad_ae_status", self._h, ctypes.c_void_p(aligned), self._ws.numel() - (aligned - base),
             stream_ptr())

    def workspace(self, B, k=1):
        need = int(self._lib.mmad_ae_workspace_bytes(self._h, int(B), int(k)))
        if need < 0:
            raise _native.NativeError("workspace size query failed")
        if self._ws is None or self._ws.numel() < need:
            # zeroed: the split-K control words must start at zero
            self._ws = torch.zeros(need + 256, dtype=torch.uint8, device=self.device)
        base = self._ws.data_ptr()
        aligned = (base + 255) // 256 * 256
        return ctypes.c_void_p(aligned), need

    @staticmethod
    def _as_input(x, width):
        x = x.reshape(x.shape[0], -1)
        if x.dtype != torch.float32:
            x = x.float()
        if x.stride(-1) != 1:
            x = x.contiguous()
        if x.shape[1] != width:
            raise ValueError(f"input width {x.shape[1]} != model input size {width}")
        return x

    # ----------------------------------------------------------------- ops
    def train_step(self, x, k=1, eps=None, seed=0, offset=0, beta_kl=0.0, loss_out=None):
        """AutoEncoder.step forward+backward: grads into self.grads; returns the
        device loss tensor [1] (no host sync)."""
        self._require(x)
        x = self._as_input(x, self.enc_widths[0])
        B = x.shape[0]
        self.sync_shadow()
        ws, nb = self.workspace(B, k)
        if loss_out is None:
            loss_out = torch.empty(1, device=self.device, dtype=torch.float32)
        if eps is not None:
            eps = eps.contiguous().float()
            assert eps.numel() == k * B * self.btl
        self.gen += 1
        call("mmad_ae_train_fwd_bwd", self._h, ptr(x), x.stride(0), B, int(k), ptr(eps),
             int(seed), int(offset), float(beta_kl), ptr(loss_out), ws, nb, stream_ptr())
        return loss_out

    def train_step_fused(self, x, lr=1e-3, betas=(0.9, 0.999), adam_eps=1e-8, k=1, eps=None,
                         seed=0, offset=0, beta_kl=0.0, loss_out=None):
        """Whole step with per-layer Adam overlapped on the side stream
        (mmad_ae_train_step); returns the device loss tensor [1]."""
        self._require(x)
        x = self._as_input(x, self.enc_widths[0])
        B = x.shape[0]
        self.sync_shadow()
        ws, nb = self.workspace(B, k)
        if loss_out is None:
            loss_out = torch.empty(1, device=self.device, dtype=torch.float32)
        if eps is not None:
            eps = eps.contiguous().float()
            assert eps.numel() == k * B * self.btl
        self.adam_step_count += 1
        self.gen += 1
        # eager multi-stream schedule by default.  SCHEDULE["train_graph"] replays
        # one captured hipGraph per step instead (mmad_ae_train_step_graph);
        # measured slower on ROCm 7 (profiles/r02e_host.log: host 377 vs 325
        # us/step, GPU 675 vs 524 us/step at C2), so it stays opt-in
        fn = "mmad_ae_train_step_graph" if self.use_graph else "mmad_ae_train_step"
        call(fn, self._h, ptr(x), x.stride(0), B, int(k), ptr(eps), int(seed),
             int(offset), float(beta_kl), float(lr), float(betas[0]), float(betas[1]),
             float(adam_eps), int(self.adam_step_count), ptr(loss_out), ws, nb, stream_ptr())
        self._mark_synced()
        return loss_out

    def backward(self, dxh, B):
        """loss.backward() after forward(train_bn=True) on the same workspace."""
        self._require(dxh)
        ws, nb = self.workspace(B, 1)
        call("mmad_ae_backward", self._h, ptr(dxh), dxh.stride(0), int(B), ws, nb, stream_ptr())

    def adam(self, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, step=None):
        if step is None:
            self.adam_step_count += 1
            step = self.adam_step_count
        call("mmad_ae_adam", self._h, float(lr), float(betas[0]), float(betas[1]), float(eps),
             int(step), stream_ptr())
        self._mark_synced()

    def adam_range(self, off, n, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, step=1):
        """Adam on the parameter range [off, off + n) (mmad_ae_adam_range) on
        the current stream; the caller counts the step."""
        call("mmad_ae_adam_range", self._h, float(lr), float(betas[0]), float(betas[1]), float(eps),
             int(step), int(off), int(n), stream_ptr())

    def dw_events(self, on=True):
        call("mmad_ae_dw_events", self._h, int(bool(on)))

    def wait_dw(self, layer, stream):
        """`stream` waits for the last train_step's dW GEMM of `layer` and its
        bwd-data GEMM (needs dw_events(True) before that step)."""
        call("mmad_ae_wait_dw", self._h, int(layer), stream_ptr(stream))

    def dw_plan(self):
        """Weight buckets in backward order: [(offset, length, lowest layer)]."""
        cap = len(self.enc_widths) + len(self.dec_widths)
        off, n, lo = (ctypes.c_int64 * cap)(), (ctypes.c_int64 * cap)(), (ctypes.c_int * cap)()
        cnt = _native.load().mmad_ae_dw_plan(self._h, cap, off, n, lo)
        if cnt < 0:
            _native.check(cnt, "mmad_ae_dw_plan")
        return [(int(off[i]), int(n[i]), int(lo[i])) for i in range(cnt)]

    def forward(self, x, train_bn=False, want_xhat=True, want_loss=False):
        self._require(x)
        x = self._as_input(x, self.enc_widths[0])
        B = x.shape[0]
        self.sync_shadow()
        ws, nb = self.workspace(B, 1)
        xh = torch.empty((B, self.dec_widths[-1]), device=self.device) if want_xhat else None
        loss = torch.empty(1, device=self.device) if want_loss else None
        self.gen += 1
        call("mmad_ae_forward", self._h, ptr(x), x.stride(0), B, int(bool(train_bn)), ptr(xh),
             self.dec_widths[-1], ptr(loss), ws, nb, stream_ptr())
        return xh, loss

    def score(self, x, want_diffs=False, nap_out=None):
        """Per-window squared-diff sums [n_enc+1, B] (and the concatenated diffs
        [B, sum widths] if asked) -- reconstruction_aggregation.get_diffs.
        nap_out (fp32 [>=B], with a fit attached by set_nap): also the NAP
        scores, from the same pass (mmad_ae_score_nap)."""
        self._require(x)
        x = self._as_input(x, self.enc_widths[0])
        B = x.shape[0]
        self.sync_shadow()
        ws, nb = self.workspace(B, 1)
        lsq = torch.empty((self.n_enc + 1, B), device=self.device)
        diffs = None
        if want_diffs:
            diffs = torch.empty((B, self.diff_width()), device=self.device)
        self.gen += 1
        if nap_out is not None:
            if want_diffs:
                raise ValueError("score: nap_out and want_diffs exclude each other")
            self._check_nap_out(nap_out, B)
            call("mmad_ae_score_nap", self._h, ptr(x), x.stride(0), B, ptr(lsq), ptr(nap_out), ws, nb,
                 stream_ptr())
            return lsq, None
        call("mmad_ae_score", self._h, ptr(x), x.stride(0), B, ptr(lsq), ptr(diffs), ws, nb,
             stream_ptr())
        return lsq, diffs

    def _check_nap_out(self, nap_out, n):
        if nap_out.device != self.device or nap_out.dtype != torch.float32 or nap_out.dim() != 1 \
                or nap_out.stride(0) != 1 or nap_out.shape[0] < n:
            raise ValueError("nap_out must be a contiguous fp32 [>=N] tensor on the model device")

    def score_stream(self, x, batch, out, graph=True, nap_out=None):
        """Whole-dataset scoring pass (mmad_ae_score_stream): x [N, D] fp32 on
        this device, out [n_enc+1, >=N] fp32 with unit column stride.  With
        graph=True the pass is captured once and replayed as one hipGraph.
        nap_out (fp32 [>=N], with a fit attached by set_nap): the pass also
        writes the NAP scores (mmad_ae_score_nap_stream)."""
        self._require(x)
        x = self._as_input(x, self.enc_widths[0])
        N = x.shape[0]
        if out.device != self.device or out.dtype != torch.float32 or out.stride(1) != 1 \
                or out.shape[0] != self.n_enc + 1 or out.shape[1] < N:
            raise ValueError("score_stream: out must be fp32 [n_enc+1, >=N] on the model device")
        self.sync_shadow()
        B = min(int(batch), N)
        ws, nb = self.workspace(B, 1)
        self.gen += 1
        if nap_out is not None:
            self._check_nap_out(nap_out, N)
            call("mmad_ae_score_nap_stream", self._h, ptr(x), x.stride(0), N, B, ptr(out),
                 out.stride(0), ptr(nap_out), ws, nb, 1 if graph else 0, stream_ptr())
            return out
        call("mmad_ae_score_stream", self._h, ptr(x), x.stride(0), N, B, ptr(out), out.stride(0),
             ws, nb, 1 if graph else 0, stream_ptr())
        return out

    def nap_fit_stream(self, x, batch, start=0, end=None, state=None):
        """The NAP fit of the diff layers [start, end) over the windows x
        [N, D] (fp32, on this device), accumulated batch by batch from the
        scoring pass (mmad_ae_nap_fit_stream): the train diffs are never
        materialised.  Returns ({'mu_r', 'v', 'mu_s', 'var'}, the fit state
        buffer: its column sums and Gram sit at mmad_nap_fit_state_layout's
        offsets from its first 256-byte aligned address)."""
        self._require(x)
        x = self._as_input(x, self.enc_widths[0])
        widths = self.diff_widths()
        end = len(widths) if end is None else int(end)
        start = int(start)
        if not 0 <= start < end <= len(widths):
            raise ValueError(f"nap_fit_stream: bad layer range [{start}, {end}) of {len(widths)} diff layers")
        N = x.shape[0]
        if N < 2:
            raise ValueError("NAP fit needs N >= 2 windows, got %d" % N)
        W = sum(widths[start:end])
        R = min(N, W)
        B = min(int(batch), N)
        self.sync_shadow()
        need = int(self._lib.mmad_ae_nap_fit_workspace_bytes(self._h, B, start, end))
        if need < 0:
            raise _native.NativeError("NAP fit workspace size query failed")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.zeros(need + 256, dtype=torch.uint8, device=self.device)
        ws = ctypes.c_void_p((self._ws.data_ptr() + 255) // 256 * 256)
        sb = int(self._lib.mmad_nap_fit_state_bytes(W))
        if state is None or state.numel() < sb + 256:
            state = torch.empty(sb + 256, dtype=torch.uint8, device=self.device)
        sp = ctypes.c_void_p((state.data_ptr() + 255) // 256 * 256)
        out = {"mu_r": torch.empty(W, device=self.device), "v": torch.empty((W, R), device=self.device),
               "mu_s": torch.empty(R, device=self.device), "var": torch.empty(R, device=self.device)}
        self.gen += 1
        call("mmad_ae_nap_fit_stream", self._h, start, end, ptr(x), x.stride(0), N, B, ptr(out["mu_r"]),
             ptr(out["v"]), ptr(out["mu_s"]), ptr(out["var"]), sp, sb, ws, need, stream_ptr())
        return out, state

    @staticmethod
    def _online_sfx(rows):
        if rows not in (16, 64):
            raise ValueError(f"online scoring: rows={rows!r} (16 or 64)")
        return "" if rows == 16 else "64"

    def online_state(self, rows=16):
        """A state buffer for online_score (mmad_ae_online_state_bytes, or
        _bytes64 for rows=64): uint8 on this device, sized for the handle as it
        stands (dtype, attached fit); the caller keeps it and passes it to
        every call with the same ``rows``."""
        need = int(getattr(self._lib, "mmad_ae_online_state_bytes" + self._online_sfx(rows))(self._h))
        if need < 0:
            raise _native.NativeError("online state size query failed")
        return torch.zeros(need + 256, dtype=torch.uint8, device=self.device)

    def group_sq(self, d, bounds, out=None, thresholds=None, flags=None):
        """Mean square of the column groups [bounds[g], bounds[g+1]) of d
        (mmad_group_sq): d fp32 [N, >= bounds[-1]] on this device with unit
        column stride (any row stride), bounds G + 1 ascending columns.
        Returns out fp32 [G, N] (given: [>= G, >= N], unit column stride);
        flags uint8 of the same shape (optional) = out > thresholds[g]
        (fp32 [G] device tensor; None: flags 0)."""
        self._require(d)
        if d.dtype != torch.float32 or d.dim() != 2 or d.stride(1) != 1:
            raise ValueError("group_sq: d must be fp32 [N, W] with unit column stride")
        bounds = [int(b) for b in bounds]
        G, N = len(bounds) - 1, d.shape[0]
        if out is None:
            out = torch.empty((max(G, 0), N), device=self.device)
        for name, t, dt in (("out", out, torch.float32), ("flags", flags, torch.uint8)):
            if t is not None and (t.device != d.device or t.dtype != dt or t.dim() != 2 or t.stride(1) != 1
                                  or t.shape[0] < G or t.shape[1] < N):
                raise ValueError(f"group_sq: {name} must be {dt} [>= G, >= N] with unit column stride")
        self._check_group_thresholds(thresholds, G, "group_sq")
        call("mmad_group_sq", N, ptr(d), d.stride(0), (ctypes.c_int * len(bounds))(*bounds), G,
             ptr(thresholds), ptr(out), out.stride(0), ptr(flags), flags.stride(0) if flags is not None else 0,
             stream_ptr())
        return out

    def _check_group_thresholds(self, thresholds, G, what):
        if thresholds is not None and (thresholds.device != self.device or thresholds.dtype != torch.float32
                                       or not thresholds.is_contiguous() or thresholds.numel() < G):
            raise ValueError(f"{what}: group thresholds must be contiguous fp32 [G] on the model device")

    def online_groups_state(self, rows=16):
        """The second buffer of a grouped online_score call
        (mmad_ae_online_groups_bytes): uint8 on this device, [rows, Kp0] fp32
        worth, where the pass leaves d0 when no attached fit stores it."""
        self._online_sfx(rows)
        need = int(self._lib.mmad_ae_online_groups_bytes(self._h, int(rows)))
        if need < 0:
            raise _native.NativeError("online groups buffer size query failed")
        return torch.zeros(need + 256, dtype=torch.uint8, device=self.device)

    def online_score(self, x, B, out, state, flags=None, thresholds=None, start=0, end=None,
                     graph=True, rows=16, groups=None, group_out=None, group_flags=None,
                     group_thresholds=None, groups_state=None):
        """Scores of B <= rows windows now (mmad_ae_online_score; rows=64:
        mmad_ae_online_score64): x fp32 [>=B, D] on this device, out fp32
        [n_enc+4, rows] (layer_sq rows, BASE, SAP, NAP), flags uint8 [3, rows]
        and thresholds fp32 [3] optional device tensors, state from
        online_state(rows).  With graph=True a repeated call (the same
        tensors) replays one captured hipGraph.
        groups (None: the call above, untouched): G + 1 ascending input
        columns; the pass then also writes the per-group mean of d0^2 into
        group_out fp32 [G, rows] (every column: >= B as 0) and group_flags
        uint8 [G, rows] (optional) = group_out > group_thresholds[g] (fp32 [G],
        optional), through mmad_ae_online_score_groups; groups_state from
        online_groups_state(rows)."""
        sfx = self._online_sfx(rows)
        self._require(x)
        if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or \
                x.shape[1] != self.enc_widths[0]:
            raise ValueError("online_score: x must be row-major fp32 [>=B, D] on the model device")
        if int(B) > x.shape[0]:
            raise ValueError(f"online_score: B={B} > the {x.shape[0]} rows of x")
        if out.device != self.device or out.dtype != torch.float32 or not out.is_contiguous() \
                or tuple(out.shape) != (self.n_enc + 4, rows):
            raise ValueError(f"online_score: out must be contiguous fp32 [n_enc+4, {rows}] on the model device")
        if flags is not None and (flags.device != self.device or flags.dtype != torch.uint8
                                  or not flags.is_contiguous() or tuple(flags.shape) != (3, rows)):
            raise ValueError(f"online_score: flags must be contiguous uint8 [3, {rows}] on the model device")
        if thresholds is not None and (thresholds.device != self.device or thresholds.dtype != torch.float32
                                       or not thresholds.is_contiguous() or thresholds.numel() != 3):
            raise ValueError("online_score: thresholds must be contiguous fp32 [3] on the model device")
        self.sync_shadow()
        base = state.data_ptr()
        aligned = (base + 255) // 256 * 256
        end = self.n_enc + 2 if end is None else int(end)
        if groups is None:
            call("mmad_ae_online_score" + sfx, self._h, ptr(x), x.stride(0), int(B), int(start), end,
                 ptr(thresholds), ptr(out), ptr(flags), ctypes.c_void_p(aligned),
                 state.numel() - (aligned - base), 1 if graph else 0, stream_ptr())
            return out
        bounds = [int(b) for b in groups]
        G = len(bounds) - 1
        for name, t, dt in (("group_out", group_out, torch.float32), ("group_flags", group_flags, torch.uint8)):
            if t is not None and (t.device != self.device or t.dtype != dt or not t.is_contiguous()
                                  or tuple(t.shape) != (G, rows)):
                raise ValueError(f"online_score: {name} must be contiguous {dt} [G, {rows}] on the model device")
        self._check_group_thresholds(group_thresholds, G, "online_score")
        gbase = groups_state.data_ptr() if groups_state is not None else 0
        galigned = (gbase + 255) // 256 * 256
        call("mmad_ae_online_score_groups", self._h, ptr(x), x.stride(0), int(B), int(start), end,
             ptr(thresholds), ptr(out), ptr(flags), ctypes.c_void_p(aligned),
             state.numel() - (aligned - base), 1 if graph else 0, stream_ptr(), int(rows),
             (ctypes.c_int * len(bounds))(*bounds), G, ptr(group_thresholds), ptr(group_out), ptr(group_flags),
             ctypes.c_void_p(galigned) if groups_state is not None else None,
             groups_state.numel() - (galigned - gbase) if groups_state is not None else 0)
        return out

    def online_tick(self, args, graph=True):
        """One sensor tick from device-resident raw buffers to scores
        (mmad_ae_online_tick): args a _native.TickArgs whose buffers the caller
        keeps alive (online.OnlineScorer.bind_sensors fills one, once).  With
        graph=True a repeated call replays one captured hipGraph."""
        self.sync_shadow()
        call("mmad_ae_online_tick", self._h, ctypes.byref(args), 1 if graph else 0, stream_ptr())

    def diff_widths(self):
        return [self.enc_widths[0]] + self.enc_widths[1:]

    def diff_width(self):
        return sum(self.diff_widths())


class _Snapshot:
    """CPU/host copy of the flat buffers used while moving devices."""

    def __init__(self, ae):
        for name in ("params", "grads", "exp_avg", "exp_avg_sq", "running"):
            setattr(self, name, getattr(ae, name).detach().clone())
