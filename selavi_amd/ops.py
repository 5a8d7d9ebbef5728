"""Thin Python wrappers over the C ABI (include/selavi_hip.h).  torch is used only to own device
memory and streams; every numeric op below is a hand-written HIP kernel in libselavi_hip.so."""
import ctypes
import os

import numpy as np
import torch

from ._lib import C, ptr, stream


def _f32(*shape, device):
    return torch.empty(*shape, dtype=torch.float32, device=device)


# The kernels address a tensor through one buffer descriptor with 32-bit byte offsets (csrc/conv_common.hpp:read_geom):
# a conv whose input or output exceeds this many bytes is run in batch slices (ConvPlan.chunks).  BASELINE configs[4]
# (128 clips x 32 frames per GPU: 7.4 GB layer-1 tensors) needs it; tests lower it to exercise the path on small tensors.
CONV_BUF_LIMIT = int(os.environ.get("SELAVI_CONV_BUF_LIMIT", str(0xFFFFFFF0)))


class ConvPlan:
    """Geometry + device tables of one convolution layer for a given input shape.

    Mirrors ``nn.Conv3d(Cin, Cout, k, stride, padding, bias=False)`` (2-D convs: T = kt = 1)."""

    _cache = {}

    def __init__(self, Bn, Cin, Ti, Hi, Wi, Cout, k, stride, pad, device):
        kt, kh, kw = k
        st, sh, sw = stride
        pt, ph, pw = pad
        To = (Ti + 2 * pt - kt) // st + 1
        Ho = (Hi + 2 * ph - kh) // sh + 1
        Wo = (Wi + 2 * pw - kw) // sw + 1
        self.in_shape = (Bn, Cin, Ti, Hi, Wi)
        self.out_shape = (Bn, Cout, To, Ho, Wo)
        self.Cin, self.Cout, self.taps = Cin, Cout, kt * kh * kw
        self.device = device
        self.count = float(Bn * To * Ho * Wo)          # elements per channel of the output
        self.P_out = To * Ho * Wo
        self.P_in = Ti * Hi * Wi
        self.chunks = None
        per_clip = 4 * max(Cin * Ti * Hi * Wi, Cout * To * Ho * Wo)
        if per_clip >= CONV_BUF_LIMIT:
            raise ValueError(f"one clip of {per_clip} bytes exceeds the conv buffer limit {CONV_BUF_LIMIT}")
        n_slices = -(-Bn // ((CONV_BUF_LIMIT - 1) // per_clip))
        if n_slices > 1:                               # batch slices, each a plan of its own (clips are independent)
            base, rem = divmod(Bn, n_slices)
            self.chunks, b0 = [], 0
            for i in range(n_slices):
                sz = base + (1 if i < rem else 0)
                self.chunks.append((b0, b0 + sz, ConvPlan.get((sz, Cin, Ti, Hi, Wi), Cout, k, stride, pad, device)))
                b0 += sz
            first = self.chunks[0][2]
            self.gp, self.geom = first.gp, first.geom  # weight layouts do not depend on the batch size
            self.wf_elems, self.wt_elems = first.wf_elems, first.wt_elems
            self.nblk = sum(c[2].nblk for c in self.chunks)
            self.cfg_fwd = self.cfg_dgrad = self.cfg_wgrad = 0
            return
        self.geom = np.array([Bn, Cin, Ti, Hi, Wi, Cout, To, Ho, Wo, kt, kh, kw, st, sh, sw, pt, ph, pw],
                             dtype=np.int32)
        self.gp = self.geom.ctypes.data
        tf = np.empty(C.slv_conv_table_len(self.gp, 0), dtype=np.int32)
        C.slv_conv_table(self.gp, 0, tf.ctypes.data)
        td = np.empty(C.slv_conv_table_len(self.gp, 1), dtype=np.int32)
        C.slv_conv_table(self.gp, 1, td.ctypes.data)
        self.tab_fwd = torch.from_numpy(tf).to(device)
        self.tab_dgrad = torch.from_numpy(td).to(device)
        self.wf_elems = C.slv_conv_wf_elems(self.gp)   # > 0: the forward conv reads tap-major weights
        self.wt_elems = C.slv_conv_wt_elems(self.gp)
        self.set_configs(0, 0, 0)
        if benchmark:
            # the key names the arithmetic EXPLICITLY and carries the key-scheme version: bare keys meant "x3" in round 4 and
            # "native" in round 5 -- entries of either scheme are simply never found (retuned), and a configuration the
            # library rejects for this arithmetic (an mf = 1 tile on a split-operand layer) is retuned instead of raised
            key = ",".join(str(int(v)) for v in self.geom) + ",k3," + conv_arithmetic()
            hit = _tune_cache().get(key)
            if hit is not None:
                try:
                    self.set_configs(*hit)
                except ValueError:
                    hit = None
                    self.set_configs(0, 0, 0)
            if hit is None:
                _autotune(self)
                _tune_cache()[key] = [self.cfg_fwd, self.cfg_dgrad, self.cfg_wgrad]
                _tune_cache_save()

    def set_configs(self, cfg_fwd, cfg_dgrad, cfg_wgrad):
        """Launch configurations (0 = built-in heuristic) and the scratch sizes that follow from them."""
        if self.chunks is not None:
            raise ValueError("a sliced plan has no launch configuration of its own: configure its slices")
        self.cfg_fwd, self.cfg_dgrad, self.cfg_wgrad = int(cfg_fwd), int(cfg_dgrad), int(cfg_wgrad)
        self.nblk = C.slv_conv_fwd_nblk(self.gp, self.cfg_fwd)
        if self.nblk <= 0:
            raise ValueError(f"invalid forward launch configuration {self.cfg_fwd:#x}")
        self.ws_fwd = C.slv_conv_fwd_ws_bytes(self.gp, self.cfg_fwd)       # split-K scratch, 0 if unsplit
        self.ws_dgrad = C.slv_conv_dgrad_ws_bytes(self.gp, self.cfg_dgrad)
        self.bnr_slots = C.slv_conv_dgrad_bnr_slots(self.gp, self.cfg_dgrad)
        self.ws_bytes = C.slv_conv_wgrad_ws_bytes(self.gp, self.cfg_wgrad)

    def candidates(self, op):
        if self.chunks is not None:
            return []
        buf = np.empty(128, dtype=np.int32)
        n = C.slv_conv_configs(self.gp, op, buf.ctypes.data, buf.size)
        return [int(v) for v in buf[:n]]

    @classmethod
    def get(cls, in_shape, Cout, k, stride, pad, device):
        key = (tuple(in_shape), Cout, tuple(k), tuple(stride), tuple(pad), str(device))
        p = cls._cache.get(key)
        if p is None:
            p = cls._cache[key] = cls(*in_shape, Cout, k, stride, pad, device)
        return p


def set_conv_arithmetic(mode):
    """"x3" (default): the fp32 convs run on the bf16 matrix cores with operands split exactly into three bf16 pieces, six
    partial products, fp32 accumulation (csrc/igemm3.hpp); "native": the fp32-input MFMA kernels (csrc/igemm.hpp).
    Plans (weight-image sizes, launch configurations) depend on it: they are dropped."""
    assert mode in ("x3", "native")
    C.slv_conv_set_arithmetic(1 if mode == "x3" else 0)
    ConvPlan._cache.clear()


def conv_arithmetic():
    return "x3" if C.slv_conv_get_arithmetic() else "native"


def plan_for(xin, conv):
    """The plan of conv layer ``conv`` (nn.Conv holder) applied to ``xin`` -- the engine's entry (ops16 has its own)."""
    return ConvPlan.get(tuple(xin.shape), conv.out_channels, conv.kernel3, conv.stride3, conv.padding3, xin.device)


FUSE_BNR = True          # the backward-data epilogue can form the source BatchNorm's backward partial sums


# Per-layer-shape timing of the launch configurations at plan creation -- the counterpart of
# `cudnn.benchmark = True` (/root/reference/main.py:187).  Off by default (deterministic heuristics);
# selavi_amd.train / bench.py switch it on.  SELAVI_BENCHMARK=0/1 overrides.
benchmark = os.environ.get("SELAVI_BENCHMARK", "0") == "1"
_tune_log = []


def set_benchmark(flag):
    global benchmark
    if "SELAVI_BENCHMARK" not in os.environ:
        benchmark = bool(flag)


# Optional persistence of the tuned configurations (SELAVI_TUNE_CACHE=<json path>): a restarted job
# skips the timing pass and -- since the K-split choice fixes the summation order -- reproduces the
# previous run's arithmetic exactly.
_tune_cache_dict = None


def _tune_cache():
    global _tune_cache_dict
    if _tune_cache_dict is None:
        _tune_cache_dict = {}
        path = os.environ.get("SELAVI_TUNE_CACHE")
        if path and os.path.exists(path):
            import json
            with open(path) as f:
                _tune_cache_dict = {k: [int(x) for x in v] for k, v in json.load(f).items()}
    return _tune_cache_dict


def _tune_cache_save():
    path = os.environ.get("SELAVI_TUNE_CACHE")
    if path:
        import json
        tmp = f"{path}.{os.getpid()}.tmp"
        with open(tmp, "w") as f:
            json.dump(_tune_cache_dict, f, indent=0, sort_keys=True)
        os.replace(tmp, path)


def _time_call(fn, reps=3):
    """Mean device time of fn() in ms: one warm call, then enough repetitions for >= ~2 ms of timed work
    (small launches are noisy), best of two such groups."""
    fn()
    best = None
    for _ in range(2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        t = e0.elapsed_time(e1) / reps
        if best is None:
            reps = int(min(20, max(reps, 2.0 / max(t, 1e-3))))
        best = t if best is None else min(best, t)
    return best


def _autotune(plan):
    """Time every candidate configuration of the three GEMMs of this layer on scratch tensors and keep
    the fastest.  Summation order inside a K-split differs between configurations, so results are
    reproducible only for a fixed choice -- same caveat as cudnn.benchmark."""
    dev = plan.device
    x = torch.randn(plan.in_shape, device=dev)
    w = torch.randn(plan.Cout, plan.Cin * plan.taps, device=dev) * 0.05
    ss = torch.stack([torch.rand(plan.Cin, device=dev) + 0.5, torch.randn(plan.Cin, device=dev) * 0.1]).contiguous()
    dy = torch.randn(plan.out_shape, device=dev)
    wf, wt = conv_w_transform(plan, w)
    best = [0, 0, 0]
    times = [None, None, None]   # (best ms, heuristic ms)
    for op in range(3):
        for cfg in [0] + plan.candidates(op):
            cfgs = [plan.cfg_fwd, plan.cfg_dgrad, plan.cfg_wgrad]
            cfgs[op] = cfg
            plan.set_configs(*cfgs)
            if op == 0:
                t = _time_call(lambda: conv_fwd(plan, x, w, in_ss=ss, in_relu=True, wf=wf))
            elif op == 1:
                t = _time_call(lambda: conv_dgrad(plan, dy, wt))
            else:
                t = _time_call(lambda: conv_wgrad(plan, dy, x, in_ss=ss, in_relu=True))
            if times[op] is None:
                times[op] = (t, t)
            elif t < times[op][0] * 0.97:       # 3 % hysteresis in favour of the earlier candidate
                times[op] = (t, times[op][1])
                best[op] = cfg
        cfgs = [plan.cfg_fwd, plan.cfg_dgrad, plan.cfg_wgrad]
        cfgs[op] = best[op]
        plan.set_configs(*cfgs)
    _tune_log.append((plan.in_shape, plan.Cout, tuple(best), tuple((round(a, 4), round(b, 4)) for a, b in times)))


_ws_cache = {}


def workspace(nbytes, device):
    """Grow-only split-K scratch buffer, one per (device, stream): calls on one stream are ordered, the two
    trunks run on different streams and must not share it."""
    # the current stream OF THAT DEVICE (device.index is None for a bare "cuda": the current device then); the raw getter: 8 us per
    # public current_stream call
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, stream(idx))
    t = _ws_cache.get(key)
    if t is None or t.numel() * 4 < nbytes:
        t = _ws_cache[key] = torch.empty(max(nbytes // 4 + 1, 1 << 20), dtype=torch.float32, device=device)
    return t


def conv_fwd(plan, x, w, in_ss=None, in_relu=False, want_stats=True, wf=None, out=None):
    """y = conv(relu?(x*s+h)); returns (y, stat_sum, stat_sq) with stats [Cout][nblk] partials.
    wf: tap-major forward weights from conv_w_transform (made on the fly when the layer needs them)."""
    if plan.wf_elems and wf is None:
        wf, _ = conv_w_transform(plan, w, need_wt=False)
    if plan.chunks is not None:
        y = _f32(*plan.out_shape, device=x.device)
        parts = []
        for b0, b1, sub in plan.chunks:
            parts.append(conv_fwd(sub, x[b0:b1], w, in_ss, in_relu, want_stats, wf, out=y[b0:b1]))
        if not want_stats:
            return y, None, None
        return y, torch.cat([p_[1] for p_ in parts], 1), torch.cat([p_[2] for p_ in parts], 1)   # [Cout][sum nblk]
    y = out if out is not None else _f32(*plan.out_shape, device=x.device)
    ssum = ssq = None
    if want_stats:
        ssum = _f32(plan.Cout, plan.nblk, device=x.device)
        ssq = _f32(plan.Cout, plan.nblk, device=x.device)
    ws = workspace(plan.ws_fwd, x.device) if plan.ws_fwd else None
    probe = _probe is not None and _probe["plan"] is plan and (in_ss is not None) == _probe["prologue"]
    if probe:          # bench.py: HIP events around THIS launch, on the stream it runs on, inside the training step
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    C.slv_conv_fwd(plan.gp, ptr(x), ptr(w), ptr(wf), ptr(plan.tab_fwd), ptr(in_ss), int(in_relu), ptr(y), ptr(ssum),
                   ptr(ssq), ptr(ws), plan.ws_fwd, plan.cfg_fwd, stream())
    if probe:
        e1.record()
        _probe["events"].append((e0, e1))
    return y, ssum, ssq


_probe = None


class probe_conv_fwd:
    """``with ops.probe_conv_fwd(plan, prologue=True) as p: step()`` -- every forward launch of ``plan`` (with / without the
    BatchNorm + ReLU prologue) inside the block is bracketed by HIP events on its own stream; ``p.ms()`` lists the durations
    after a synchronize.  Measurement only (bench.py's live ``roofline.in_step``): two event records per probed launch."""

    def __init__(self, plan, prologue=True):
        self.state = dict(plan=plan, prologue=prologue, events=[])

    def __enter__(self):
        global _probe
        _probe = self.state
        return self

    def __exit__(self, *exc):
        global _probe
        _probe = None

    def ms(self):
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in self.state["events"]]


def conv_w_transform(plan, w, need_wf=True, need_wt=True):
    """Per-step re-layouts of the weights (one read of w): (wf, wt) -- see include/selavi_hip.h."""
    wf = _f32(plan.wf_elems, device=w.device) if (need_wf and plan.wf_elems) else None
    wt = _f32(plan.wt_elems, device=w.device) if need_wt else None
    if wf is not None or wt is not None:
        C.slv_conv_w_transform(plan.gp, ptr(w), ptr(wf), ptr(wt), stream())
    return wf, wt


def conv_wt_transform(plan, w):
    return conv_w_transform(plan, w, need_wf=False)[1]


# Off by default: measured in the step (tools/step16_bench.py, two interleaved pairs, one box) the one launch is 0.3 ms SLOWER
# than the ~70 it replaces (fp32 30.16 / 30.22 ms against 29.82 / 29.95; bf16 12.34 against 12.23) although the forward alone
# gains 0.1 ms: an image made right in front of its conv is still in the 256 MB Infinity Cache when the conv's workgroups stream
# it, the images of the one launch at the head of the trunk (190 + 190 MB) are not.  SELAVI_BATCH_W_IMAGES=1 switches it on.
BATCH_W_IMAGES = os.environ.get("SELAVI_BATCH_W_IMAGES", "0") == "1"


class WeightImages:
    """The per-step weight re-layouts of a whole trunk in ONE launch (slv_conv_w_transform_jobs) instead of one per conv layer
    (~70 launches of the fp32 step).  Life cycle, per (trunk, input shape, mode): the first pass runs the per-layer entry
    point and RECORDS (plan, weight, need_wt) of every conv it meets (``note``); ``build`` then allocates persistent image
    buffers, asks the library for the job descriptors (slv_conv_w_jobs) and copies the table to the device once; from the
    next pass on ``run`` makes every image with one launch at the head of the trunk and ``get`` hands them out.  Layers
    without split-operand images (the 3 / 1-channel stems, the native arithmetic) stay on the per-layer path.
    The images are rewritten by every pass that calls ``run`` (weights change at every optimizer step); a backward pass
    reads the backward-data images its own forward made."""

    def __init__(self):
        self.rec, self.seen = [], set()
        self.ent = None                   # id(weight) -> (plan, wf, wt)
        self.table, self.njobs, self.blocks = None, 0, 0

    def note(self, plan, w, need_wt):
        if id(w) not in self.seen and plan.chunks is None:
            self.seen.add(id(w))
            self.rec.append((plan, w, need_wt))

    def build(self, device):
        words = C.slv_conv_w_job_words()
        jobs, ent = [], {}
        for plan, w, need_wt in self.rec:
            wf = _f32(plan.wf_elems, device=device) if plan.wf_elems else None
            wt = _f32(plan.wt_elems, device=device) if need_wt else None
            if wf is None and wt is None:
                continue
            buf = np.zeros(1024 * words, dtype=np.int32)
            n = C.slv_conv_w_jobs(plan.gp, ptr(w), ptr(wf), ptr(wt), buf.ctypes.data, 1024)
            if n <= 0:
                continue                  # (this layer keeps slv_conv_w_transform)
            jobs.append(buf[:n * words])
            ent[id(w)] = (plan, wf, wt, w)
        self.rec = None
        self.ent = ent
        if jobs:
            tab = np.concatenate(jobs)
            self.table = torch.from_numpy(tab).to(device)
            self.njobs = tab.size // words
            self.blocks = 0               # the library's choice (jobs are equal: 16 384 slots each)
        return self

    @property
    def ready(self):
        return self.ent is not None

    def run(self):
        if self.table is not None:
            C.slv_conv_w_transform_jobs(ptr(self.table), self.njobs, self.blocks, stream())

    def get(self, plan, w, need_wt):
        e = self.ent.get(id(w)) if self.ent is not None else None
        if e is None or e[0] is not plan or e[3] is not w or (need_wt and e[2] is None):
            return None
        return e[1], (e[2] if need_wt else None)


def conv_dgrad(plan, dy, wt, x_out=None, bwd5=None, relu=False, addend=None, out=None, bnr=None):
    """dx = conv_transpose(dy) (+ addend).  bnr = (x, scale_shift, mean_invstd) of the layer that produced
    this conv's input: the kernel epilogue then also emits that BatchNorm's backward partial sums and
    (dx, part) is returned -- pass `part` to bn_bwd."""
    dx = out if out is not None else _f32(*plan.in_shape, device=dy.device)
    if bwd5 is not None:     # BN backward of the conv's own output: materialised, then a plain dgrad
        dy = bn_bwd_apply(dy, x_out, bwd5, relu, out=torch.empty_like(dy))
    if plan.chunks is not None:
        parts = []
        for b0, b1, sub in plan.chunks:
            r = conv_dgrad(sub, dy[b0:b1], wt, addend=None if addend is None else addend[b0:b1], out=dx[b0:b1],
                           bnr=None if bnr is None else (bnr[0][b0:b1], bnr[1], bnr[2]))
            parts.append(r[1] if bnr is not None else None)
        return dx if bnr is None else (dx, torch.cat(parts, 1))                    # [Cin][sum slots][2]
    ws = workspace(plan.ws_dgrad, dy.device) if plan.ws_dgrad else None
    part = rx = rss = rmi = None
    if bnr is not None:
        rx, rss, rmi = bnr
        part = _f32(plan.Cin, plan.bnr_slots, 2, device=dy.device)
    C.slv_conv_dgrad(plan.gp, ptr(dy), ptr(wt), ptr(plan.tab_dgrad), ptr(dx), ptr(addend), ptr(rx), ptr(rss), ptr(rmi),
                     ptr(part), ptr(ws), plan.ws_dgrad, plan.cfg_dgrad, stream())
    return dx if bnr is None else (dx, part)


def conv_wgrad(plan, dy, x_in, x_out=None, bwd5=None, a_relu=False, in_ss=None, in_relu=False, out=None):
    dw = out if out is not None else _f32(plan.Cout, plan.Cin * plan.taps, device=dy.device)
    if bwd5 is not None:
        dy = bn_bwd_apply(dy, x_out, bwd5, a_relu, out=torch.empty_like(dy))
    if plan.chunks is not None:
        n = len(plan.chunks)
        slices = _f32(n, plan.Cout, plan.Cin * plan.taps, device=dy.device)
        for i, (b0, b1, sub) in enumerate(plan.chunks):
            conv_wgrad(sub, dy[b0:b1], x_in[b0:b1], in_ss=in_ss, in_relu=in_relu, out=slices[i])
        C.slv_sum_slices(ptr(slices), ptr(dw), n, dw.numel(), stream())
        return dw
    ws = workspace(plan.ws_bytes, dy.device) if plan.ws_bytes else None
    C.slv_conv_wgrad(plan.gp, ptr(dy), ptr(x_in), ptr(in_ss), int(in_relu), ptr(plan.tab_fwd), ptr(dw),
                     ptr(ws), plan.ws_bytes, plan.cfg_wgrad, stream())
    return dw


def gemm_nt(A, B, bias=None, out=None):
    M, K = A.shape
    N = B.shape[0]
    Cm = out if out is not None else _f32(M, N, device=A.device)
    C.slv_gemm_nt(ptr(A), ptr(B), ptr(bias), ptr(Cm), M, N, K, N, stream())
    return Cm


# ---------------------------------------------------------------------------------- BatchNorm
def _allreduce(t, where):
    """where: comm.NativeComm (RCCL call on the current stream) or a torch.distributed group."""
    from .comm import allreduce_sum_
    allreduce_sum_(t, where)


def _native(sync):
    from .comm import NativeComm
    return sync[0] if isinstance(sync[0], NativeComm) else None


def _span(kind):
    """comm.span: HIP events around an exchange while a comm.diagnostics() block is open, otherwise nothing."""
    from . import comm
    return comm.span(kind)


def bn_train_finalize(ssum, ssq, count, gamma, beta, rmean, rvar, momentum, eps, sync=None):
    """conv-epilogue partials -> (mean_invstd [2][C], scale_shift [2][C]); updates running stats.
    ``sync`` = (group, world_count): SyncBN -- sums are all-reduced, count is the global count."""
    Cc = gamma.numel()
    dev = gamma.device
    mi = _f32(2, Cc, device=dev)
    ss = _f32(2, Cc, device=dev)
    if sync is None:
        C.slv_bn_stats_finalize(ptr(ssum), ptr(ssq), ssum.shape[1], float(count), ptr(gamma), ptr(beta), ptr(rmean),
                                ptr(rvar), float(momentum), float(eps), ptr(mi), ptr(ss), Cc, stream())
        return mi, ss
    sums = torch.empty(2 * Cc, dtype=torch.float64, device=dev)
    EXCHANGES[0] += 1
    comm = _native(sync)
    with _span("syncbn"):
        if comm is not None:        # one library call, one stream: partials -> sums -> RCCL all-reduce -> finalize
            C.slv_bn_sync_finalize(comm.h, ptr(ssum), ptr(ssq), ssum.shape[1], float(count), ptr(gamma), ptr(beta), ptr(rmean),
                                   ptr(rvar), float(momentum), float(eps), ptr(mi), ptr(ss), Cc, ptr(sums), stream())
            return mi, ss
        C.slv_bn_partials_to_sums(ptr(ssum), ptr(ssq), ssum.shape[1], Cc, ptr(sums), stream())
        _allreduce(sums, sync[0])
        count = count * sync[1]
        C.slv_bn_finalize(ptr(sums), float(count), ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), float(momentum),
                          float(eps), ptr(mi), ptr(ss), Cc, stream())
    return mi, ss


EXCHANGES = [0]        # SyncBN exchanges issued by this process (tests count them per step)


def bn_train_finalize_many(items, sync):
    """Several BatchNorms whose statistics are complete at the same point of the schedule (the last conv of a residual
    block and its downsample conv: nothing consumes either before the block tail) finalised behind ONE exchange:
    items = [(ssum, ssq, count, gamma, beta, rmean, rvar, momentum, eps), ...] -> [(mean_invstd, scale_shift), ...].
    The 2C fp64 sums of all items travel in one buffer; kernels and arithmetic are those of bn_train_finalize."""
    with _span("syncbn"):
        return _bn_train_finalize_many(items, sync)


def _bn_train_finalize_many(items, sync):
    dev = items[0][3].device
    tot = sum(2 * it[3].numel() for it in items)
    sums = torch.empty(tot, dtype=torch.float64, device=dev)
    o, views = 0, []
    for ssum, ssq, count, gamma, *_ in items:
        Cc = gamma.numel()
        v = sums[o:o + 2 * Cc]
        C.slv_bn_partials_to_sums(ptr(ssum), ptr(ssq), ssum.shape[1], Cc, ptr(v), stream())
        views.append(v)
        o += 2 * Cc
    _allreduce(sums, sync[0])
    EXCHANGES[0] += 1
    outs = []
    for v, (ssum, ssq, count, gamma, beta, rmean, rvar, momentum, eps) in zip(views, items):
        Cc = gamma.numel()
        mi, ss = _f32(2, Cc, device=dev), _f32(2, Cc, device=dev)
        C.slv_bn_finalize(ptr(v), float(count * sync[1]), ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), float(momentum),
                          float(eps), ptr(mi), ptr(ss), Cc, stream())
        outs.append((mi, ss))
    return outs


def bn_eval_params(gamma, beta, rmean, rvar, eps):
    Cc = gamma.numel()
    mi = _f32(2, Cc, device=gamma.device)
    ss = _f32(2, Cc, device=gamma.device)
    C.slv_bn_eval_params(ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), float(eps), ptr(mi), ptr(ss), Cc, stream())
    return mi, ss


def bn_act(x, ss, res=None, res_ss=None, relu=True):
    Bn, Cc = x.shape[0], x.shape[1]
    P = x.numel() // (Bn * Cc)
    out = torch.empty_like(x)
    C.slv_bn_act(ptr(x), ptr(ss), ptr(res), ptr(res_ss), int(relu), ptr(out), Bn, Cc, P, stream())
    return out


def bn_bwd(g, x, mi, gamma, ss_mask=None, v_mask=None, x2=None, mi2=None, gamma2=None, ss2=None, sync=None,
           dgamma=None, dbeta=None, dgamma2=None, dbeta2=None, part=None):
    """BN backward reductions for the BN whose input is ``x`` and upstream gradient ``g``.

    mask: ``ss_mask`` (the BN's own scale/shift -> ReLU mask on its output) or ``v_mask`` (block
    output tensor; the masked gradient is materialised and returned) or none.  Optional second BN
    (downsample branch) sharing the same masked gradient.  Returns (bwd5, bwd5_2, g_masked)."""
    Bn, Cc = x.shape[0], x.shape[1]
    P = x.numel() // (Bn * Cc)
    dev = x.device
    gout = part2 = None
    if part is not None:        # partial sums already formed by the producing dgrad's epilogue (ss_mask case)
        assert ss_mask is not None and v_mask is None and x2 is None
        ns = part.shape[1]
    else:
        ns = C.slv_bn_bwd_nsplit(Bn, Cc, P)
        part = _f32(Cc, ns, 2, device=dev)
        part2 = _f32(Cc, ns, 2, device=dev) if x2 is not None else None
        gout = torch.empty_like(g) if v_mask is not None else None
        C.slv_bn_bwd_reduce(ptr(g), ptr(x), ptr(mi), ptr(ss_mask), ptr(v_mask), ptr(x2), ptr(mi2), ptr(gout),
                            ptr(part), ptr(part2), Bn, Cc, P, ns, stream())
    outs = bn_bwd_finish(part, part2, ns, float(Bn * P), mi, gamma, ss_mask, mi2, gamma2, sync, dgamma, dbeta,
                         dgamma2, dbeta2)
    return outs[0], outs[1], gout


def bn_bwd_finish(part, part2, ns, count, mi, gamma, ss_mask, mi2, gamma2, sync, dgamma, dbeta, dgamma2, dbeta2):
    """Slice partials [C][ns][2] -> folded BatchNorm-backward coefficients bwd5 [5][C] (+ dgamma, dbeta); SyncBN: the
    fp64 sums are all-reduced in between.  Shared by the fp32 (N,C,T,H,W) and the bf16 channels-last reductions."""
    if sync is None:
        return _bn_bwd_finish(part, part2, ns, count, mi, gamma, ss_mask, mi2, gamma2, sync, dgamma, dbeta, dgamma2, dbeta2)
    with _span("syncbn"):
        return _bn_bwd_finish(part, part2, ns, count, mi, gamma, ss_mask, mi2, gamma2, sync, dgamma, dbeta, dgamma2, dbeta2)


def _bn_bwd_finish(part, part2, ns, count, mi, gamma, ss_mask, mi2, gamma2, sync, dgamma, dbeta, dgamma2, dbeta2):
    Cc = gamma.numel()
    dev = gamma.device
    comm = _native(sync) if sync is not None else None
    local_count = count
    if sync is not None:
        count *= sync[1]
    jobs = [(part, mi, gamma, ss_mask, dgamma, dbeta), (part2, mi2, gamma2, None, dgamma2, dbeta2)]
    if sync is not None and part2 is not None:
        # the block's last BatchNorm and its downsample BatchNorm: both sets of sums behind ONE exchange
        sums = torch.empty(4 * Cc, dtype=torch.float64, device=dev)
        for k, (pt_, *_r) in enumerate(jobs):
            C.slv_bn_bwd_sums(ptr(pt_), ns, Cc, ptr(sums[2 * Cc * k:2 * Cc * (k + 1)]), stream())
        _allreduce(sums, sync[0])
        EXCHANGES[0] += 1
        outs = []
        for k, (pt_, mi_, ga_, ss_, dg_, db_) in enumerate(jobs):
            b5 = _f32(5, Cc, device=dev)
            C.slv_bn_bwd_finalize(ptr(sums[2 * Cc * k:2 * Cc * (k + 1)]), count, ptr(ga_), ptr(mi_), ptr(ss_), ptr(b5), ptr(dg_),
                                  ptr(db_), 0, Cc, stream())
            outs.append(b5)
        return outs
    outs = []
    for (pt_, mi_, ga_, ss_, dg_, db_) in jobs:
        if pt_ is None:
            outs.append(None)
            continue
        b5 = _f32(5, Cc, device=dev)
        if sync is not None:
            EXCHANGES[0] += 1
        if comm is not None:
            sums = torch.empty(2 * Cc, dtype=torch.float64, device=dev)
            C.slv_bn_bwd_sync_finalize(comm.h, ptr(pt_), ns, local_count, ptr(ga_), ptr(mi_), ptr(ss_), ptr(b5), ptr(dg_),
                                       ptr(db_), 0, Cc, ptr(sums), stream())
            outs.append(b5)
            continue
        if sync is None:
            C.slv_bn_bwd_sums_finalize(ptr(pt_), ns, count, ptr(ga_), ptr(mi_), ptr(ss_), ptr(b5), ptr(dg_), ptr(db_),
                                       0, Cc, stream())
            outs.append(b5)
            continue
        sums = torch.empty(2 * Cc, dtype=torch.float64, device=dev)
        C.slv_bn_bwd_sums(ptr(pt_), ns, Cc, ptr(sums), stream())
        _allreduce(sums, sync[0])
        C.slv_bn_bwd_finalize(ptr(sums), count, ptr(ga_), ptr(mi_), ptr(ss_), ptr(b5), ptr(dg_), ptr(db_), 0, Cc,
                              stream())
        outs.append(b5)
    return outs


def bn_bwd_apply(g, x, b5, relu, out=None):
    """dXout = A1*mask*g + A2 + A3*x (in place over g by default)."""
    Bn, Cc = x.shape[0], x.shape[1]
    P = x.numel() // (Bn * Cc)
    out = g if out is None else out
    C.slv_bn_bwd_apply(ptr(g), ptr(x), ptr(b5), int(relu), ptr(out), Bn, Cc, P, stream())
    return out


def avgpool_fwd(v):
    Bn, Cc = v.shape[0], v.shape[1]
    P = v.numel() // (Bn * Cc)
    out = _f32(Bn, Cc, device=v.device)
    C.slv_avgpool_fwd(ptr(v), ptr(out), Bn * Cc, P, stream())
    return out


def avgpool_bwd(dout, like):
    Bn, Cc = like.shape[0], like.shape[1]
    P = like.numel() // (Bn * Cc)
    dv = torch.empty_like(like)
    C.slv_avgpool_bwd(ptr(dout), ptr(dv), Bn * Cc, P, stream())
    return dv


def bnrelu_maxpool_fwd(x, ss):
    Bn, Cc, T, H, W = x.shape
    assert T == 1
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    out = _f32(Bn, Cc, 1, Ho, Wo, device=x.device)
    idx = torch.empty(Bn, Cc, 1, Ho, Wo, dtype=torch.uint8, device=x.device)
    C.slv_bnrelu_maxpool_fwd(ptr(x), ptr(ss), ptr(out), ptr(idx), Bn, Cc, H, W, stream())
    return out, idx


def maxpool_bwd(dout, idx, in_shape):
    Bn, Cc, T, H, W = in_shape
    dy = _f32(*in_shape, device=dout.device)
    C.slv_maxpool_bwd(ptr(dout), ptr(idx), ptr(dy), Bn, Cc, H, W, stream())
    return dy


# ---------------------------------------------------------------------------------- pointer tables
class PtrArray:
    """Host array of device pointers (``const void* const*`` in the C ABI)."""

    def __init__(self, tensors):
        self.n = len(tensors)
        self.arr = (ctypes.c_void_p * max(self.n, 1))(*[t.data_ptr() for t in tensors])
        self.keep = list(tensors)

    @property
    def p(self):
        return ctypes.addressof(self.arr)


def sgd_step(params, grads, bufs, lr, momentum, wd, first):
    n = len(params)
    pa, ga, ba = PtrArray(params), PtrArray(grads), PtrArray(bufs)
    sizes = (ctypes.c_int64 * n)(*[p.numel() for p in params])
    C.slv_sgd_step(pa.p, ga.p, ba.p, ctypes.addressof(sizes), n, float(lr), float(momentum), float(wd), int(first),
                   stream())


# ---------------------------------------------------------------------------------- video retrieval (csrc/retrieval.hip)
def pool222(x, op="max", channels=None):
    """MaxPool3d / AvgPool3d((2, 2, 2), stride 2) + Flatten (reference src/retrieval_utils.py:86-98) -> fp32 [N, C*To*Ho*Wo]
    in the view(N, -1) order of an N,C,T,H,W tensor.  x: fp32 N,C,T,H,W, or bf16 channels-last [N,T,H,W,Cp] whose first
    ``channels`` channels are real (the 16-bit engine's layout)."""
    if op not in ("max", "avg"):
        raise ValueError(f"pool op {op!r}: max | avg")
    if x.dim() != 5:
        raise ValueError(f"pool222 takes a 5-D tensor, got {tuple(x.shape)}")
    x = x.contiguous()
    if x.dtype == torch.bfloat16:
        N, T, H, W, Cp = x.shape
        Cc = channels if channels is not None else Cp
    elif x.dtype == torch.float32:
        N, Cc, T, H, W = x.shape
    else:
        raise ValueError(f"pool222 takes fp32 N,C,T,H,W or bf16 channels-last, got {x.dtype}")
    To, Ho, Wo = T // 2, H // 2, W // 2
    if min(To, Ho, Wo) == 0:
        raise ValueError(f"pool222: input T,H,W = {T},{H},{W} gives a pooled extent of 0")
    out = _f32(N, Cc * To * Ho * Wo, device=x.device)
    if x.dtype == torch.bfloat16:
        C.slv_pool222_cl16(ptr(x), ptr(out), N, T, H, W, Cc, Cp, int(op == "avg"), stream())
    else:
        C.slv_pool222_f32(ptr(x), ptr(out), N, Cc, T, H, W, int(op == "avg"), stream())
    return out


def row_sqnorm(x):
    """fp32 [R, D] -> [R] sums of squares."""
    x = x.contiguous()
    out = _f32(x.shape[0], device=x.device)
    C.slv_row_sqnorm(ptr(x), x.shape[0], x.shape[1], ptr(out), stream())
    return out


def segment_mean(x, vid_indices, normalize=True):
    """The averaging of average_features (reference src/retrieval_utils.py:290-330) on the device.

    x: fp32 [R, D] clip features; vid_indices: [R] video ids.  Videos come in the order of their first appearance (the
    reference's dict insertion order); each video's rows are summed in clip order (optionally each divided by its L2 norm
    first) and divided by their count.  -> (mean [V, D], video ids [V] int64, first row of each video [V] int64,
    squared norms of the means [V])."""
    x = x.contiguous()
    R, D = x.shape
    vid = vid_indices.to(device=x.device, dtype=torch.int64)
    if vid.shape != (R,):
        raise ValueError(f"segment_mean: {R} rows but video indices of shape {tuple(vid.shape)}")
    uniq, inv = torch.unique(vid, return_inverse=True)
    V = uniq.shape[0]
    rows = torch.arange(R, device=x.device)
    first = torch.full((V,), R, dtype=torch.int64, device=x.device).scatter_reduce_(0, inv, rows, reduce="amin")
    order = torch.argsort(first)                          # videos by first appearance
    rank = torch.empty_like(order)
    rank[order] = torch.arange(V, device=x.device)
    seg = rank[inv]
    perm = torch.sort(seg, stable=True).indices.to(torch.int32)     # rows of each video, in clip order
    offsets = torch.zeros(V + 1, dtype=torch.int32, device=x.device)
    offsets[1:] = torch.cumsum(torch.bincount(seg, minlength=V), 0).to(torch.int32)
    out = _f32(V, D, device=x.device)
    sq = _f32(V, device=x.device)
    ws = _f32(R, device=x.device) if normalize else None
    C.slv_segment_mean(ptr(x), R, D, ptr(perm), ptr(offsets), V, int(bool(normalize)), ptr(ws), ptr(out), ptr(sq), stream())
    return out, uniq[order], first[order], sq


KNN_MAX_K = 64
# cap of the [chunk, N_bank] fp32 dot-product buffer of knn (the query rows run in chunks under it)
KNN_CHUNK_BYTES = int(os.environ.get("SELAVI_KNN_CHUNK_BYTES", str(256 << 20)))


def knn(queries, bank, k, q_sqnorm=None, bank_sqnorm=None, max_chunk_bytes=None):
    """Brute-force Euclidean k nearest neighbours (NearestNeighbors(k).kneighbors, reference src/retrieval_utils.py:410-440).

    queries fp32 [Q, D], bank fp32 [N, D] -> (d2 fp32 [Q, k], idx int32 [Q, k]): squared distances ascending, ties to the
    lower bank index.  The dot products come from slv_gemm_nt in query chunks whose [chunk, N] buffer stays under
    ``max_chunk_bytes``; slv_knn_select completes d^2 = |q|^2 + |t|^2 - 2 q.t (clamped at 0) and selects."""
    queries, bank = queries.contiguous(), bank.contiguous()
    Q, D = queries.shape
    N = bank.shape[0]
    if bank.shape[1] != D:
        raise ValueError(f"knn: queries of dimension {D}, bank of dimension {bank.shape[1]}")
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"knn: k = {k} must be in [1, {KNN_MAX_K}]")
    if k > N:
        raise ValueError(f"knn: Expected n_neighbors <= n_samples, but n_samples = {N}, n_neighbors = {k}")
    qs = row_sqnorm(queries) if q_sqnorm is None else q_sqnorm.contiguous()
    ts = row_sqnorm(bank) if bank_sqnorm is None else bank_sqnorm.contiguous()
    cap = KNN_CHUNK_BYTES if max_chunk_bytes is None else int(max_chunk_bytes)
    chunk = max(1, min(Q, cap // (4 * N)))
    dots = _f32(chunk, N, device=queries.device)
    d2 = _f32(Q, k, device=queries.device)
    idx = torch.empty(Q, k, dtype=torch.int32, device=queries.device)
    for r0 in range(0, Q, chunk):
        m = min(chunk, Q - r0)
        C.slv_gemm_nt(ptr(queries[r0:r0 + m]), ptr(bank), 0, ptr(dots), m, N, D, N, stream())
        C.slv_knn_select(ptr(dots), N, m, N, ptr(qs[r0:r0 + m]), ptr(ts), k, ptr(d2[r0:r0 + m]), ptr(idx[r0:r0 + m]),
                         stream())
    return d2, idx


# ---------------------------------------------------------------------------------- fine-tuning (csrc/finetune.hip)
class FtHeadSaved:
    """What ft_head_fwd keeps for ft_head_bwd: the rows after the L2 normalisation, their norms, the BatchNorm mean /
    invstd, the dropout draw (mask tensor or Philox (seed, offset)) and the forward's dlogits."""
    __slots__ = ("u", "norms", "mi", "mask", "seed", "offset", "p", "drop", "dlogits", "l2", "bn", "train")


def ft_head_fwd(x, W, bias, bn_mod=None, l2=False, train=False, p=0.0, mask=None, dropout_stream=None, target=None,
                need_dlogits=False):
    """Finetune_Model's head (reference finetune_video.py:83-92) in one launch at B <= 64: [L2 norm] -> [BatchNorm1d]
    -> [dropout, train only] -> Linear, with the cross-entropy / accuracy epilogue when ``target`` is given.

    bn_mod: the BatchNorm holder (weight, bias, running_mean, running_var, momentum, eps) or None; mask: injected keep
    mask [B, 512] (else Philox on ``dropout_stream()``'s (seed, offset)).  -> (logits [B, K], loss [] or None,
    correct [2] (correct@1, correct@5 counts) or None, FtHeadSaved)."""
    x = x.contiguous()
    B, D = x.shape
    K = W.shape[0]
    if D != 512 or W.shape[1] != 512:
        raise ValueError(f"ft_head_fwd: the head takes 512-d features, got x {tuple(x.shape)}, W {tuple(W.shape)}")
    dev = x.device
    drop = bool(train and p > 0)
    s = FtHeadSaved()
    s.l2, s.bn, s.train, s.drop, s.p = bool(l2), bn_mod is not None, bool(train), drop, float(p)
    s.mask, s.seed, s.offset = None, 0, 0
    if drop:
        if mask is not None:
            s.mask = mask.to(device=dev, dtype=torch.float32).contiguous()
            if s.mask.shape != (B, 512):
                raise ValueError(f"dropout mask of shape {tuple(s.mask.shape)}, expected {(B, 512)}")
        else:
            s.seed, s.offset = dropout_stream()
    logits = _f32(B, K, device=dev)
    s.u, s.norms, s.mi = _f32(B, 512, device=dev), _f32(B, device=dev), _f32(2, 512, device=dev)
    loss = correct = ws = None
    s.dlogits = None
    tg = None
    if target is not None:
        tg = target.to(device=dev, dtype=torch.int64).contiguous()
        if tg.shape != (B,):
            raise ValueError(f"ft_head_fwd: {B} rows but targets of shape {tuple(tg.shape)}")
        loss, correct, ws = _f32(1, device=dev), _f32(2, device=dev), _f32(3 * B, device=dev)
        if need_dlogits:
            s.dlogits = _f32(B, K, device=dev)
    bm = bn_mod
    C.slv_ft_head_fwd(ptr(x), ptr(W), ptr(bias), ptr(bm.weight if bm is not None else None),
                      ptr(bm.bias if bm is not None else None), ptr(bm.running_mean if bm is not None else None),
                      ptr(bm.running_var if bm is not None else None), ptr(s.mask), s.seed, s.offset, float(p), ptr(tg),
                      ptr(logits), ptr(s.u), ptr(s.norms), ptr(s.mi), ptr(s.dlogits), ptr(ws), ptr(loss), ptr(correct),
                      B, K, int(s.l2), int(s.bn), int(s.train), int(drop),
                      float(bm.momentum) if bm is not None else 0.1, float(bm.eps) if bm is not None else 1e-5, stream())
    return logits, (loss.view(()) if loss is not None else None), correct, s


def ft_head_bwd(s, W, bn_mod, dlogits=None, gout=None):
    """Backward of ft_head_fwd: dz = dlogits + gout * (the forward's dlogits).  -> (dfeat [B, 512], dW, db, dgamma,
    dbeta) (dgamma / dbeta None without BatchNorm)."""
    B = s.u.shape[0]
    K = W.shape[0]
    dev = s.u.device
    dz = dlogits.contiguous() if dlogits is not None else None
    dls = s.dlogits if gout is not None else None
    g = gout.to(dtype=torch.float32).contiguous().reshape(1) if dls is not None else None
    dW, db, dfeat = _f32(K, 512, device=dev), _f32(K, device=dev), _f32(B, 512, device=dev)
    dga = dbe = None
    if s.bn:
        dga, dbe = _f32(512, device=dev), _f32(512, device=dev)
    ws = _f32(2 * B * 512, device=dev) if B > 64 else None
    bm = bn_mod
    C.slv_ft_head_bwd(ptr(dz), ptr(dls), ptr(g), ptr(s.u), ptr(s.norms), ptr(s.mi), ptr(W),
                      ptr(bm.weight if s.bn else None), ptr(bm.bias if s.bn else None), ptr(s.mask), s.seed, s.offset,
                      float(s.p), ptr(dW), ptr(db), ptr(dga), ptr(dbe), ptr(dfeat), ptr(ws), B, K, int(s.l2), int(s.bn),
                      int(s.train), int(s.drop), stream())
    return dfeat, dW, db, dga, dbe


def topk_correct(scores, target):
    """[2] float32 device tensor: how many rows of ``scores`` [N, K] have their int64 target in the top 1 / top 5, under
    the deterministic rule #{j: z_j > z_t} + #{j < t: z_j == z_t} < k (ties go to the lower class index)."""
    scores = scores.contiguous()
    if scores.dtype != torch.float32 or scores.dim() != 2:
        raise ValueError(f"topk_correct takes fp32 [N, K] scores, got {scores.dtype} {tuple(scores.shape)}")
    N, K = scores.shape
    tg = target.to(device=scores.device, dtype=torch.int64).contiguous().reshape(-1)
    if tg.shape[0] != N:
        raise ValueError(f"topk_correct: {N} rows but {tg.shape[0]} targets")
    out = _f32(2, device=scores.device)
    C.slv_topk_correct(ptr(scores), N, K, ptr(tg), ptr(out), stream())
    return out


def sgd_step_grouped(params, grads, bufs, lrs, wds, momenta, firsts):
    """slv_sgd_step with per-tensor lr / weight decay / momentum / first-step flag (48 tensors per launch)."""
    n = len(params)
    pa, ga, ba = PtrArray(params), PtrArray(grads), PtrArray(bufs)
    sizes = (ctypes.c_int64 * n)(*[p.numel() for p in params])
    lr_a, wd_a, mu_a = ((ctypes.c_float * n)(*[float(v) for v in vs]) for vs in (lrs, wds, momenta))
    fi = (ctypes.c_int32 * n)(*[int(bool(v)) for v in firsts])
    C.slv_sgd_step_grouped(pa.p, ga.p, ba.p, ctypes.addressof(sizes), ctypes.addressof(lr_a), ctypes.addressof(wd_a),
                           ctypes.addressof(mu_a), ctypes.addressof(fi), n, stream())


def adam_step(params, grads, exp_avgs, exp_avg_sqs, step_sizes, bc2_sqrts, wds, beta1, beta2, eps):
    """torch.optim.Adam's update with per-tensor step size lr / (1 - beta1^step), sqrt(1 - beta2^step) and weight decay
    (48 tensors per launch)."""
    n = len(params)
    pa, ga, ma, va = PtrArray(params), PtrArray(grads), PtrArray(exp_avgs), PtrArray(exp_avg_sqs)
    sizes = (ctypes.c_int64 * n)(*[p.numel() for p in params])
    ss, bc, wd = ((ctypes.c_float * n)(*[float(v) for v in vs]) for vs in (step_sizes, bc2_sqrts, wds))
    C.slv_adam_step(pa.p, ga.p, ma.p, va.p, ctypes.addressof(sizes), ctypes.addressof(ss), ctypes.addressof(bc),
                    ctypes.addressof(wd), n, float(beta1), float(beta2), float(eps), stream())
