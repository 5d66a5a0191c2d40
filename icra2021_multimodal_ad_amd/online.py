"""Online scoring: the anomaly scores of the latest few windows, now.

The reference's deployment loop (test_file/realtime_tester.py:291-309,
get_realtime_dataloader) fuses the latest 10 sensor windows and asks for their
scores, over and over.  ``OnlineScorer`` is the object that loop calls: it owns
a fixed device input buffer [rows, D], the outputs, the threshold buffer and the
native state (mmad_ae_online_state_bytes), so every call after the first is one
replayed hipGraph of about 20 short weight-streaming launches
(mmad_ae_online_score; DESIGN.md §4 "Online scoring").  ``rows`` is 16 (the
default) or 64 (mmad_ae_online_score64: up to four 16-row tiles against one
weight stream, every window's scores the bits of the 16-row path's).  More
windows than ``rows`` are the batch route's
(reconstruction_aggregation.score_windows).

``groups`` adds per-modality scores: the mean squared reconstruction error of
named column ranges of the input row (HSR_Net.modality_columns() for the fused
row), from one more launch in the same graph (mmad_ae_online_score_groups).
The ranges are CONTIGUOUS: each starts where the one before it ends (the
operator takes ascending bounds); a caller who wants a gap names the gap as a
group of its own and ignores its row.

``bind_sensors`` / ``tick`` run a whole sensor tick -- raw queues to scores --
as one host-to-device copy and one replayed graph (mmad_ae_online_tick: the
MFCC launches, mmad_hsr_fuse_raw with norm_vec folded into its loads, the
pass above).  ``score_sensors`` stays the route for a microphone queue that is
still filling (DESIGN.md §4 "Sensor tick in one graph").
"""
import ctypes

import numpy as np
import torch

from . import metric
from ._native import MAX_GROUPS

ROWS = 16            # the default row capacity
ROW_CAPACITIES = (16, 64)
METHODS = ("base", "sap", "nap")


def group_bounds(groups, width):
    """(names, bounds) of ``groups``: a mapping name -> (c0, c1) or a list of
    (c0, c1) pairs (named by position), ordered by c0, contiguous, inside
    [0, width].  bounds: the G + 1 ascending columns mmad_group_sq takes."""
    items = list(groups.items()) if hasattr(groups, "items") else list(enumerate(groups))
    items = sorted(((n, (int(c[0]), int(c[1]))) for n, c in items), key=lambda it: it[1][0])
    if not 1 <= len(items) <= MAX_GROUPS:
        raise ValueError(f"OnlineScorer: {len(items)} groups (1..{MAX_GROUPS})")
    bounds = [items[0][1][0]]
    for name, (c0, c1) in items:
        if c0 != bounds[-1]:
            raise ValueError(f"OnlineScorer: group {name!r} starts at column {c0}, the one before it ends at "
                             f"{bounds[-1]}: groups are contiguous (name a gap as a group of its own)")
        if c1 <= c0:
            raise ValueError(f"OnlineScorer: group {name!r} is empty ({c0}, {c1})")
        bounds.append(c1)
    if bounds[0] < 0 or bounds[-1] > width:
        raise ValueError(f"OnlineScorer: groups span [{bounds[0]}, {bounds[-1]}) outside the {width} input columns")
    return tuple(n for n, _ in items), bounds


_reciprocal = {}


def device_divides_by_reciprocal(device):
    """Whether torch on ``device`` computes fp32 ``tensor / python_scalar`` as
    the product with the rounded reciprocal of the scalar (its device kernels
    do; the quotients of 0, 2, .., 510 by 255 tell: 126 of the 256 are one ulp
    off the division), False when it is the IEEE quotient.  Probed once a device;
    normalised_sensors goes through that operator, so ``bind_sensors`` has the
    tick's kernel form the quotient the same way."""
    device = torch.device(device)
    if device not in _reciprocal:
        v = 2 * np.arange(256, dtype=np.float32)
        got = (torch.from_numpy(v).to(device) / 255).cpu().numpy()
        ieee, rcp = v / np.float32(255), v * (np.float32(1) / np.float32(255))
        if np.array_equal(got, ieee):
            _reciprocal[device] = False
        elif np.array_equal(got, rcp):
            _reciprocal[device] = True
        else:
            raise RuntimeError("device_divides_by_reciprocal: torch's fp32 division by a scalar is neither the "
                               "quotient nor the reciprocal product on this device; set OnlineScorer.norm_division")
    return _reciprocal[device]


def rows_for(n_windows):
    """The row capacity for a loop that scores ``n_windows`` (None: unknown)
    windows a call: 64 for 17..64, else the 16-row default (at <= 16 windows
    the two are level within the measurement spread and the 16-row state is
    a quarter of the size: DESIGN.md §4 "Online scoring"; beyond 64 no
    capacity fits and the scorer names the batch route)."""
    return 64 if 16 < int(n_windows or 0) <= 64 else ROWS


def _aligned(buf):
    """(256-byte aligned address inside ``buf``, the bytes left from there)."""
    p = (buf.data_ptr() + 255) // 256 * 256
    return p, buf.numel() - (p - buf.data_ptr())


def _member_args(sc, a, keep):
    """One scorer's pass arguments -- SAP range, thresholds, outputs, state and
    groups -- into ``a``: a TickArgs (OnlineScorer.bind_sensors) or a
    BankMember (SensorBank); the two name these fields alike.  keep: a dict
    that holds the ctypes bounds array alive."""
    a.sap_start, a.sap_end = sc.start, sc.end
    a.thresholds, a.out, a.flags = sc.thresholds.data_ptr(), sc.out.data_ptr(), sc.flags.data_ptr()
    a.state, a.state_bytes = _aligned(sc.state)
    if sc.groups is not None:
        keep["bounds"] = (ctypes.c_int * len(sc.groups))(*sc.groups)
        a.bounds, a.G = keep["bounds"], len(sc.groups) - 1
        a.group_thresholds, a.group_out = sc.group_thresholds.data_ptr(), sc.group_out.data_ptr()
        a.group_flags = sc.group_flags.data_ptr()
        a.gstate, a.gstate_bytes = _aligned(sc.groups_state)


def _bind_front(who, x, rows, hsr_net, mic_samples, hand_dtype, depth_dtype, front_end, norm_division,
                fused_model=False):
    """What OnlineScorer.bind_sensors and SensorBank.bind_sensors share: the
    checks, the staging layout (PCM int16 [mic_samples] | hand [B][3072] | depth
    [B][1024] | force fp32 [B], every segment 256-byte aligned), its pinned
    host buffer and device twin, the MFCC buffers, the packed HSR weights, the
    ``norm_division`` probe, and a TickArgs with the front end, the fusion
    producer and the fused row's destination ``x`` [rows, >= 1728] filled in.
    fused_model: the caller's model reads the whole row (x must be 1728 wide)."""
    from . import _native
    from .data_loaders import mic_front_end
    B = int(hsr_net.batch_size)
    if B > rows:
        raise ValueError(f"{who}.bind_sensors: slicing_size {B} > {rows}; score_windows "
                         "(reconstruction_aggregation) is the batch route")
    if hsr_net.unimodal:
        raise ValueError(f"{who}.bind_sensors: the tick fuses all four streams (a fused HSR_Net)")
    kinds = {np.dtype(np.uint8): _native.SRC_U8, np.dtype(np.float32): _native.SRC_F32}
    hand_dtype, depth_dtype = np.dtype(hand_dtype), np.dtype(depth_dtype)
    if hand_dtype not in kinds or depth_dtype not in kinds:
        raise ValueError(f"{who}.bind_sensors: hand / depth of {hand_dtype} / {depth_dtype} (uint8 or float32)")
    dev = x.device
    fe = front_end or mic_front_end(device=dev)
    L = int(mic_samples)
    F = fe.frames(L)
    if F < B:
        raise ValueError(f"{who}.bind_sensors: {L} samples are {max(F, 0)} frames < the {B} windows of a tick")
    if fe.n_mfcc != 13 or (x.shape[1] != 1728 if fused_model else x.shape[1] < 1728):
        raise ValueError(f"{who}.bind_sensors: the fused row takes 13 MFCCs and a 1728-wide model")
    # the staging layout: name -> (byte offset, dtype, shape)
    seg, off = {}, 0
    for name, dt, shape in (("pcm", np.dtype(np.int16), (L,)), ("hand", hand_dtype, (B, 3072)),
                            ("depth", depth_dtype, (B, 1024)), ("force", np.dtype(np.float32), (B,))):
        seg[name] = (off, dt, shape)
        off = (off + int(np.prod(shape)) * dt.itemsize + 255) // 256 * 256
    host = torch.zeros(off, dtype=torch.uint8).pin_memory()
    raw = torch.zeros(off, dtype=torch.uint8, device=dev)
    flat = host.numpy()
    views = {k: flat[o:o + int(np.prod(s)) * dt.itemsize].view(dt).reshape(s) for k, (o, dt, s) in seg.items()}
    lib = _native.load()
    t = dict(B=B, L=L, net=hsr_net, host=host, raw=raw, views=views, copied=torch.cuda.Event(), front_end=fe,
             mfcc=torch.zeros((F, 13), device=dev), norm=torch.zeros((B, 13), device=dev),
             ws=torch.zeros(int(lib.mmad_mfcc_ws_bytes(F, fe.n_mels)), dtype=torch.uint8, device=dev),
             weights=torch.zeros(int(lib.mmad_hsr_weight_count()), device=dev))
    hsr_net.packed_weights(out=t["weights"])
    a, ptr = _native.TickArgs(), (lambda v: v.data_ptr())
    base = raw.data_ptr()
    a.pcm, a.pcm_type, a.L = base + seg["pcm"][0], _native.PCM_I16, L
    a.r, a.r_type = base + seg["hand"][0], kinds[hand_dtype]
    a.d, a.d_type = base + seg["depth"][0], kinds[depth_dtype]
    a.t = base + seg["force"][0]
    a.range_in[:] = [0, 255, 0, 255, 0, 400]        # normalised_sensors' ranges
    how = norm_division or ("reciprocal" if device_divides_by_reciprocal(dev) else "ieee")
    if how not in ("ieee", "reciprocal"):
        raise ValueError(f"{who}.norm_division={how!r} ('ieee', 'reciprocal' or None)")
    a.norm_rcp = int(how == "reciprocal")
    a.sr, a.n_fft, a.n_mels, a.n_mfcc = fe.params
    a.plan, a.plan_bytes = ptr(fe.plan), fe.plan.numel()
    a.mfcc_out, a.mfcc_out_bytes = ptr(t["mfcc"]), t["mfcc"].numel() * 4
    a.mfcc_norm, a.mfcc_norm_bytes = ptr(t["norm"]), t["norm"].numel() * 4
    a.mfcc_ws, a.mfcc_ws_bytes = ptr(t["ws"]), t["ws"].numel()
    a.hsr_weights, a.hsr_weight_count = ptr(t["weights"]), t["weights"].numel()
    a.x, a.ld_x, a.B, a.rows = ptr(x), x.stride(0), B, rows
    t["args"] = a
    return t


def _stage_queues(who, t, force_q, hand_q, depth_q, mic_q):
    """The queues of one tick into the pinned staging buffer of ``t``
    (_bind_front) with numpy, then its copy to the device on the current
    stream: the first B frames of force, hand and depth, all of mic_q (int16
    samples or the reference's list of ``bytes`` chunks)."""
    B, L, v = t["B"], t["L"], t["views"]
    if isinstance(mic_q, (bytes, bytearray, memoryview)):
        mic_q = [mic_q]
    chunks = isinstance(mic_q, (list, tuple)) and (not mic_q or isinstance(mic_q[0], (bytes, bytearray, memoryview)))
    if chunks:
        n_mic = sum(len(c) for c in mic_q) // 2
    else:
        mic_q = np.asarray(mic_q).reshape(-1)
        if mic_q.dtype != np.int16:
            raise ValueError(f"{who}.tick: PCM of dtype {mic_q.dtype} (the staging buffer holds int16)")
        n_mic = mic_q.size
    if n_mic != L:
        raise ValueError(f"{who}.tick: a mic queue of {n_mic} samples, bound to {L}; score_sensors takes "
                         "a queue that is still filling")
    qs = {}
    for name, q in (("force", force_q), ("hand", hand_q), ("depth", depth_q)):
        q = np.asarray(q)
        q = q.reshape(q.shape[0], -1) if q.ndim > 1 else q.reshape(-1, 1)
        if q.shape[0] < B:
            raise ValueError(f"{who}.tick: {name} queue of {q.shape[0]} frames < the {B} windows of a tick")
        if q.shape[1] != v[name].reshape(B, -1).shape[1]:
            raise ValueError(f"{who}.tick: {name} frames of {q.shape[1]} values")
        if v[name].dtype == np.uint8 and q.dtype != np.uint8:
            raise ValueError(f"{who}.tick: {name} queue of {q.dtype}, bound as uint8")
        qs[name] = q[:B]
    t["copied"].synchronize()            # the last tick's copy has read the staging buffer
    if chunks:
        np.copyto(v["pcm"], np.frombuffer(b"".join(mic_q), dtype=np.int16))
    else:
        np.copyto(v["pcm"], mic_q)
    for name, q in qs.items():
        np.copyto(v[name].reshape(B, -1), q, casting="same_kind")
    t["raw"].copy_(t["host"], non_blocking=True)
    t["copied"].record()


class _SharedRoutes:
    """The routes OnlineScorer and SensorBank share, on the fixed input row
    ``self.x`` [rows, W]: ``score``, ``score_frames``, ``score_sensors``,
    ``refresh_sensors`` and ``tick``.  Each class supplies ``_run(B)`` (its
    native pass on the first B rows of ``self.x``), ``_tick_native(args)`` (its
    native tick), ``_results(B)`` and ``_fuse`` (HSR_Net.forward into ``self.x``
    with the class's own refusals).  Messages carry the calling class's name."""
    front_end = None     # score_sensors' MfccFrontEnd (set one to change its settings)
    _tick = None         # bind_sensors' buffers and argument struct
    # norm_vec's quotient inside the tick, read by bind_sensors: 'ieee' (a
    # correctly rounded division, mmad_hsr_fuse_raw's), 'reciprocal' (the
    # product with fl(1 / (hi - lo))), or None: whichever of the two torch's
    # elementwise kernels compute on the scorer's device, so that ``tick``
    # returns score_sensors' bits (device_divides_by_reciprocal)
    norm_division = None
    _fused_model = False  # the tick's fused row is this object's model input (x exactly 1728 wide)

    def score(self, x):
        """x: [B <= rows, W] (W = ``self.x.shape[1]``: the model's input size,
        or the bank's row width), host or device.  OnlineScorer returns
        {'base','sap','nap','layer_sq','flags'}: views of its fixed outputs on
        the device, rewritten by the next call (copy what you keep); with
        groups also 'groups' [G, B] and 'group_flags' [G, B], rows in the order
        of ``group_names`` (ascending columns).  SensorBank returns {name:
        that scorer's dict for x[:, c0:c1]}."""
        who = type(self).__name__
        x = torch.as_tensor(x)
        x = x.reshape(x.shape[0], -1)
        B = x.shape[0]
        if B > self.rows:
            raise ValueError(f"{who}.score: {B} windows > {self.rows}; score_windows "
                             "(reconstruction_aggregation) is the batch route")
        if B < 1 or x.shape[1] != self.x.shape[1]:
            raise ValueError(f"{who}.score: x must be [1..{self.rows}, {self.x.shape[1]}], got {tuple(x.shape)}")
        self.x[:B].copy_(x, non_blocking=True)
        return self._run(B)

    def score_frames(self, hsr_net, r, d, t, m):
        """One step of get_realtime_dataloader: HSR_Net.forward (mmad_hsr_fuse)
        of the latest ``hsr_net.batch_size`` <= rows frames straight into the
        fixed input row, on the same stream, then ``score``'s pass."""
        B = int(hsr_net.batch_size)
        if B > self.rows:
            raise ValueError(f"{type(self).__name__}.score_frames: slicing_size {B} > {self.rows}; score_windows "
                             "(reconstruction_aggregation) is the batch route")
        self._fuse(hsr_net, (r, d, None, t, m), B)
        return self._run(B)

    def score_sensors(self, hsr_net, force_q, hand_q, depth_q, mic_pcm):
        """One tick of the deployment loop from the raw queues
        (get_realtime_dataloader, utils/data_loaders.py:734-737): norm_vec's
        fixed-range maps of the camera, depth and force/torque frames
        (elementwise torch), the microphone's MFCCs and their norm_vec to
        [-1, 1] over the last ``hsr_net.batch_size`` frames (mmad_mfcc, on the
        same stream, ahead of the replayed graph), then ``score_frames``.
        mic_pcm: what MfccFrontEnd takes (``self.front_end``: built on first
        use with the reference's 44.1 kHz / 0.1 s / 128 mel / 13 settings).
        This is the route for a microphone queue that is still filling;
        ``tick`` is the one-graph route."""
        from .data_loaders import mic_front_end, normalised_sensors
        dev = self.x.device
        if self.front_end is None:
            self.front_end = mic_front_end(device=dev)
        r, d, t = normalised_sensors(force_q, hand_q, depth_q, dev)
        m = self.front_end.latest(mic_pcm, int(hsr_net.batch_size))[1]
        return self.score_frames(hsr_net, r, d, t, m)

    # ---- the sensor tick as one replayed graph (mmad_ae_online_tick) ---------
    def bind_sensors(self, hsr_net, mic_samples, hand_dtype=np.uint8, depth_dtype=np.uint8, front_end=None):
        """Fix the shapes of ``tick``: the fused ``hsr_net`` (its
        ``batch_size`` = B <= rows windows a tick), a microphone queue of
        exactly ``mic_samples`` int16 samples, and the camera queues' element
        types (uint8 or float32).  Allocates one pinned host staging buffer
        and its device twin -- PCM int16 [mic_samples] | hand [B][3072] |
        depth [B][1024] | force fp32 [B], every segment 256-byte aligned --
        the MFCC outputs, the front end's workspace at its final size and the
        HSR weights, packed once (``refresh_sensors`` repacks them).
        front_end: an MfccFrontEnd (None: ``self.front_end``, else the
        reference's 44.1 kHz / 0.1 s / 128 mel / 13 settings).  A bank binds
        one set of these for all members and the fused row lands in its
        shared ``x`` (1728 wide at least); it needs no fused member: a bank of
        one 'mic' scorer is the unimodal tick."""
        t = _bind_front(type(self).__name__, self.x, self.rows, hsr_net, mic_samples, hand_dtype, depth_dtype,
                        front_end or self.front_end, self.norm_division, fused_model=self._fused_model)
        self.front_end = t["front_end"]
        if self._fused_model:              # the scorer is the tick's one member
            _member_args(self, t["args"], t)
        self._tick = t
        return self

    def refresh_sensors(self):
        """Repack the bound HSR_Net's weights into the buffer the tick's graph
        reads, after its parameters changed: the next ``tick`` sees them, no
        new capture."""
        if self._tick is None:
            raise ValueError(f"{type(self).__name__}.refresh_sensors: call bind_sensors first")
        self._tick["net"].packed_weights(out=self._tick["weights"])

    def tick(self, force_q, hand_q, depth_q, mic_q):
        """``score_sensors`` on the shapes ``bind_sensors`` fixed, as one
        host-to-device copy and one graph launch: the queues are written into
        the pinned staging buffer with numpy (the first B frames of force,
        hand and depth, as HSR_Net.forward takes them; all of mic_q: int16
        samples or the reference's list of ``bytes`` chunks), copied over on
        the current stream, and the native tick (mmad_ae_online_tick; the
        bank's mmad_online_bank_tick, for every member) replays MFCC ->
        fusion -> scoring.  Returns what ``score_sensors`` returns."""
        who, t = type(self).__name__, self._tick
        if t is None:
            raise ValueError(f"{who}.tick: call bind_sensors first")
        _stage_queues(who, t, force_q, hand_q, depth_q, mic_q)
        self._tick_native(t["args"])
        return self._results(t["B"])


class OnlineScorer(_SharedRoutes):
    # per-modality scores: off unless ``groups`` is given (then instance attributes)
    groups = None
    group_names = ()
    _fused_model = True

    def __init__(self, model, nap=None, start_layer_index=0, end_layer_index=None, thresholds=None,
                 rows=ROWS, groups=None):
        """model: an eval-mode autoencoder of the plugin surface (fp32 or bf16,
        no split-bf16 score planes).  nap: a fitted NapScorer (its fit is
        attached to ``model`` for this object's lifetime; a standalone scorer
        is taken to cover the SAP layer range) or None (no NAP score).
        start / end_layer_index: the SAP layer range as
        ``sap_from_layer_sq`` takes it.  thresholds: {'base','sap','nap'} ->
        float, or None (NaN: no flag until ``calibrate``).  rows: 16 or 64,
        the most windows a call takes (the size of every buffer here).
        groups: None, or named column ranges of the input row (a mapping name
        -> (c0, c1) or a list of pairs; contiguous, see the module text):
        ``score`` then also returns their mean squared reconstruction error
        and flags against thresholds['groups'] (name -> float)."""
        if rows not in ROW_CAPACITIES:
            raise ValueError(f"OnlineScorer: rows={rows!r} (16 or 64)")
        self.rows = rows
        nat = model._native
        model.eval()
        self.model, self.nat, self.nap = model, nat, nap
        n = nat.n_enc + 1
        self.start = int(start_layer_index)
        self.end = n + 1 if end_layer_index is None else int(end_layer_index)
        if nap is not None:
            layers = None
            if nap.model is None:          # standalone: name the layers it was fit on
                s = min(max(self.start, 0), n - 1)
                e = min(max(self.end, s + 1), n)
                layers = (s, e)
            nap.attach(model, precision="f32", layers=layers)
        dev = nat.device
        self.x = torch.zeros((rows, nat.enc_widths[0]), device=dev)
        self.out = torch.zeros((nat.n_enc + 4, rows), device=dev)
        self.flags = torch.zeros((3, rows), device=dev, dtype=torch.uint8)
        self.thresholds = torch.full((3,), float("nan"), device=dev)
        self.state = nat.online_state(rows)
        if groups is not None:
            self.group_names, self.groups = group_bounds(groups, nat.enc_widths[0])
            G = len(self.group_names)
            self.group_out = torch.zeros((G, rows), device=dev)
            self.group_flags = torch.zeros((G, rows), device=dev, dtype=torch.uint8)
            self.group_thresholds = torch.full((G,), float("nan"), device=dev)
            self.groups_state = nat.online_groups_state(rows)
        if thresholds is not None:
            self.set_thresholds(thresholds)

    def set_thresholds(self, thresholds):
        """{'base','sap','nap'} -> float (a missing one: NaN, no flag), written
        into the device buffer the pass reads: the next replay sees them.
        With groups, 'groups' -> {name: float} sets the group thresholds the
        same way (a missing name: NaN; no 'groups' entry: left as they are)."""
        t = torch.tensor([float(thresholds.get(k, float("nan"))) for k in METHODS], dtype=torch.float32)
        self.thresholds.copy_(t)
        gt = thresholds.get("groups")
        if gt is not None:
            if self.groups is None:
                raise ValueError("OnlineScorer: thresholds['groups'] on a scorer without groups")
            self.group_thresholds.copy_(torch.tensor([float(gt.get(n, float("nan"))) for n in self.group_names],
                                                     dtype=torch.float32))
        return t

    def calibrate(self, valid_scores, q=metric.F1_QUANTILE):
        """Thresholds by the quantile rule of metric.threshold_metrics
        (np.quantile(valid, q), linear) on validation scores {'base','sap','nap'}
        -> [Nv]; returns them as a dict.  With groups, 'groups' -> {name:
        [Nv]} calibrates each named group's threshold by the same rule."""
        def quantile(v):
            v = torch.as_tensor(v).reshape(-1)
            return metric.threshold_metrics(v, v[:1], np.zeros(1, np.uint8), q)[0]
        thr = {}
        for k in METHODS:
            v = valid_scores.get(k)
            if v is not None:
                thr[k] = quantile(v)
        gv = valid_scores.get("groups")
        if gv is not None:
            thr["groups"] = {n: quantile(v) for n, v in gv.items() if v is not None}
        self.set_thresholds(thr)
        return thr

    def _run(self, B):
        grouped = {} if self.groups is None else dict(
            groups=self.groups, group_out=self.group_out, group_flags=self.group_flags,
            group_thresholds=self.group_thresholds, groups_state=self.groups_state)
        self.nat.online_score(self.x, B, self.out, self.state, flags=self.flags,
                              thresholds=self.thresholds, start=self.start, end=self.end,
                              rows=self.rows, **grouped)
        return self._results(B)

    def _results(self, B):
        n_enc = self.nat.n_enc
        res = {"layer_sq": self.out[:n_enc + 1, :B], "base": self.out[n_enc + 1, :B],
               "sap": self.out[n_enc + 2, :B],
               "nap": self.out[n_enc + 3, :B] if self.nap is not None else None,
               "flags": self.flags[:, :B]}
        if self.groups is not None:
            res["groups"] = self.group_out[:, :B]
            res["group_flags"] = self.group_flags[:, :B]
        return res

    def _fuse(self, hsr_net, streams, B):
        fused = hsr_net.forward(*streams, out=self.x)
        if fused.reshape(B, -1).shape[1] != self.x.shape[1]:
            raise ValueError("OnlineScorer.score_frames: the fused row width is not the model's input size")

    def _tick_native(self, args):
        self.nat.online_tick(args)

    def close(self):
        """Detach the fit from the model."""
        if self.nap is not None:
            self.nap.detach()
            self.nap = None


# config.sensor names -> the modality keys of HSR_Net.modality_columns()
SENSOR_KEYS = {"All": None, "hand_camera": "r", "head_depth": "d", "force_torque": "t", "mic": "m"}


class SensorBank(_SharedRoutes):
    """Several OnlineScorers -- the fused detector and its unimodal siblings,
    independent models -- scored on ONE shared input row per tick, sharing
    launches (mmad_online_bank_score / _tick; DESIGN.md §4 "Sensor bank"):
    layer step l of every member is one grouped launch, the whole bank one
    replayed graph.  Each scorer keeps its own state, outputs, thresholds, fit
    and groups (``calibrate`` stays per scorer), and every scoring method
    returns {name: what that scorer's own call returns} -- views of the
    scorers' fixed outputs, bit for bit what the scorer alone computes on its
    columns.

    The bank shares one fused HSR_Net (``score_frames`` / ``score_sensors`` /
    ``tick``): there are no per-member HSR weights, so the unimodal models are
    expected to have been trained on that network's blocks of the fused row."""

    _h = None

    def __init__(self, scorers, columns=None, width=None):
        """scorers: a mapping name -> OnlineScorer or a sequence (named by
        position), 1..8 of them, of one row capacity and on one device.
        columns: the first column of the shared row each scorer reads (a
        mapping by name or a sequence; None: every scorer reads column 0);
        scorer i reads [c, c + D_i).  The native pack reads 16-byte quads, so a
        column start must be a multiple of 4.  width: the shared row's width
        (None: where the last member's columns end)."""
        from . import _native
        items = list(scorers.items()) if hasattr(scorers, "items") else list(enumerate(scorers))
        if not 1 <= len(items) <= _native.MAX_BANK:
            raise ValueError(f"SensorBank: {len(items)} scorers (1..{_native.MAX_BANK})")
        self.names = tuple(n for n, _ in items)
        self.scorers = {n: s for n, s in items}
        members = [s for _, s in items]
        if len({s.rows for s in members}) != 1:
            raise ValueError(f"SensorBank: scorers of mixed rows {[s.rows for s in members]}; one row capacity a bank")
        if len({s.x.device for s in members}) != 1:
            raise ValueError("SensorBank: scorers on different devices")
        self.rows = members[0].rows
        if columns is None:
            cols = [0] * len(members)
        elif hasattr(columns, "items"):
            cols = [int(columns[n]) for n in self.names]
        else:
            cols = [int(c) for c in columns]
        if len(cols) != len(members) or min(cols) < 0:
            raise ValueError("SensorBank: one non-negative column start per scorer")
        self.columns = {n: (c, c + s.x.shape[1]) for n, c, s in zip(self.names, cols, members)}
        dev = members[0].x.device
        self.x = torch.zeros((self.rows, max([int(width or 0)] + [c1 for _, c1 in self.columns.values()])),
                             device=dev)
        lib = _native.load()
        n = len(members)
        self._handles = (ctypes.c_void_p * n)(*[s.nat._h for s in members])
        self._col0 = (ctypes.c_int * n)(*cols)
        h = ctypes.c_void_p()
        _native.check(lib.mmad_online_bank_create(ctypes.byref(h), n, self._handles, self._col0, self.rows),
                      "mmad_online_bank_create")
        self._h, self._lib = h, lib
        self._keep = [dict() for _ in members]
        self._members = (_native.BankMember * n)()
        for sc, m, keep in zip(members, self._members, self._keep):
            _member_args(sc, m, keep)

    @classmethod
    def for_sensors(cls, hsr_net, scorers):
        """scorers: config.sensor name ('All', 'hand_camera', 'head_depth',
        'force_torque', 'mic') -> OnlineScorer; the column starts are those of
        ``hsr_net.modality_columns()`` (a fused HSR_Net), 'All' at 0."""
        cols = hsr_net.modality_columns()
        starts = {}
        for name in scorers:
            if name not in SENSOR_KEYS:
                raise ValueError(f"SensorBank.for_sensors: unknown sensor {name!r} ({', '.join(SENSOR_KEYS)})")
            key = SENSOR_KEYS[name]
            starts[name] = 0 if key is None else cols[key][0]
        return cls(scorers, starts, width=max(c1 for _, c1 in cols.values()))

    def graph_nodes(self):
        """Kernel nodes of the last captured pass (mmad_online_bank_graph_nodes)."""
        return int(self._lib.mmad_online_bank_graph_nodes(self._h))

    def graph_count(self):
        return int(self._lib.mmad_online_bank_graph_count(self._h))

    def _results(self, B):
        return {n: s._results(B) for n, s in self.scorers.items()}

    def _call(self, name, *args):
        from . import _native
        for s in self.scorers.values():
            s.nat.sync_shadow()
        _native.check(getattr(self._lib, name)(self._h, *args, _native.stream_ptr()), name)

    def _run(self, B, graph=True):
        self._call("mmad_online_bank_score", self.x.data_ptr(), self.x.stride(0), int(B), self._members,
                   1 if graph else 0)
        return self._results(B)

    def _fuse(self, hsr_net, streams, B):
        if hsr_net.unimodal or self.x.shape[1] != 1728:
            raise ValueError("SensorBank.score_frames: a fused HSR_Net and a 1728-wide shared row")
        hsr_net.forward(*streams, out=self.x)

    def _tick_native(self, args):
        self._call("mmad_online_bank_tick", ctypes.byref(args), self._members, 1)

    def close(self):
        """Drop the bank's captured graphs and native object (the scorers,
        their fits included, stay as they are: close them on their own)."""
        if self._h is not None:
            self._lib.mmad_online_bank_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
