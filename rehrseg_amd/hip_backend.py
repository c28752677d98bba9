"""Launch layer: turns torch tensors into the plain-pointer descriptors of the
C-ABI (include/rehrseg_hip.h) and launches on torch's current HIP stream.

Every activation handed to this module is a 5-D torch tensor with logical shape
(N, C, D, H, W) whose memory is NDHWC-dense (``ops.to_cl``).  PyTorch is used for
device memory and streams only; all arithmetic happens in librehrseg_hip.so.
"""
from __future__ import annotations

import ctypes as C
import os
import functools
import weakref

import torch
from torch.optim.optimizer import register_optimizer_step_post_hook as _register_step_hook

from . import lib as L

name = "hip"


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# Optional per-launch timing of the MFMA kernels (bench.py's roofline line): HIP
# events recorded on the launch stream around every gather-GEMM / wgrad launch.
_prof = None


def profile_start():
    global _prof
    _prof = []


def profile_stop(layers=False):
    """-> {family: {"flops", "seconds", "launches"}} summed over the recorded launches; layers=True: the launches one by
    one as (family, shape tag, flops, seconds) instead (tools/layer_times.py)."""
    global _prof
    rec, _prof = _prof, None
    torch.cuda.synchronize()
    if layers:
        return [(fam, tag, flops, e0.elapsed_time(e1) * 1e-3) for fam, flops, e0, e1, tag in rec or []]
    out = {}
    for fam, flops, e0, e1, _ in rec or []:
        d = out.setdefault(fam, {"flops": 0.0, "seconds": 0.0, "launches": 0})
        d["flops"] += flops
        d["seconds"] += e0.elapsed_time(e1) * 1e-3
        d["launches"] += 1
    return out


@functools.lru_cache(maxsize=4096)
def _reach(L, s, b, taps, size):
    """Number of (lattice point, tap) pairs of one axis whose source index is in bounds:
    the algorithmic work of a launch excludes taps that fall into the zero padding."""
    cnt, off0, offs, _, _ = taps
    tot = 0
    for j in range(cnt):
        c = b + off0 + offs * j
        lo = max(0, -(c // s)) if c < 0 else 0          # smallest o with o*s + c >= 0
        hi = min(L - 1, (size - 1 - c) // s) if size - 1 - c >= 0 else -1
        tot += max(0, hi - lo + 1)
    return tot


def _algo_flops(N, lattice, s, b, taps, dims, c_a, c_b):
    f = 2.0 * N * c_a * c_b
    for a in range(3):
        f *= _reach(lattice[a], s[a], b[a], tuple(taps[a]), dims[a])
    return f


class _timed:
    def __init__(self, fam, flops, tag=None):
        self.fam, self.flops, self.tag = fam, flops, tag

    def __enter__(self):
        if _prof is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if _prof is not None:
            self.e1.record()
            _prof.append((self.fam, self.flops, self.e0, self.e1, self.tag() if callable(self.tag) else self.tag))
        return False


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _taps(t):
    return L.AxisTaps(*t)


def _workspace(query, args, device, what):
    """A uint8 tensor of exactly the bytes the library's size query `query(*args)` reports; a negative answer is the
    query's error code and raises.  Callers pass ws.numel() as the byte count."""
    nbytes = int(query(*args))
    if nbytes < 0:
        L.check(nbytes, what)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _chk_dev(*ts, f64=()):
    """Every operand of the fp32 kernels must be a float32 device tensor; `f64` lists the statistics buffers
    (double accumulators) of the call."""
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise L.RehrsegHipError("librehrseg_hip.so needs device tensors (no CPU fallback)")
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise L.RehrsegHipError(f"unsupported dtype {t.dtype} (the kernels read float32, the mixed-precision "
                                    "variants bfloat16)")
    for t in f64:
        if t is None:
            continue
        if not t.is_cuda or t.dtype != torch.float64:
            raise L.RehrsegHipError("statistics buffers are float64 device tensors")


def _chk_eval(t, dtype, what, dim=None):
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or (dim is not None and t.dim() != dim):
        raise L.RehrsegHipError(f"{what}: contiguous {dtype} device tensor" + (f" of {dim} dims" if dim else "") +
                                " (no CPU fallback)")


def _fn(base, t):
    """C entry point `base`_f32 or `base`_bf16 by the dtype of activation tensor `t`."""
    name = base + ("_bf16" if t.dtype == torch.bfloat16 else "_f32")
    return getattr(L.load(), name), name


def _same_dtype(*ts):
    dts = {t.dtype for t in ts if t is not None}
    if len(dts) > 1:
        raise L.RehrsegHipError(f"activation operands of one call must share a dtype, got {sorted(map(str, dts))}")


# Small zero-initialised fp64 accumulators (per-(sample, channel) statistics, gradient reductions): every fused layer
# needs one or two per pass, and a torch.zeros() each is a 5 us fill launch -- ~90 per cfg-2 step.  They are carved out
# of a pooled chunk that is zeroed by ONE fill when it is allocated; a slice is handed out once and never reused (the
# chunk lives as long as any slice of it does), so no kernel ever sees stale values.  One pool per (device, stream): the
# fill runs on the stream that is current when the chunk is made, and only kernels of that stream may rely on it.
_zero_pool = {}
_ZERO_CHUNK = 1 << 16   # doubles (512 KB)


def zeros_f64(shape, device):
    n = 1
    for s in shape:
        n *= int(s)
    n_al = (n + 1) & ~1                                   # keep 16-byte alignment of every slice
    if n_al > _ZERO_CHUNK // 4:
        return torch.zeros(shape, dtype=torch.float64, device=device)
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)
    ent = _zero_pool.get(key)
    if ent is None or ent[1] + n_al > _ZERO_CHUNK:
        ent = [torch.zeros(_ZERO_CHUNK, dtype=torch.float64, device=device), 0]
        _zero_pool[key] = ent
    out = ent[0][ent[1]:ent[1] + n].view(shape)
    ent[1] += n_al
    return out


def new_act(N, Cc, D, H, W, like, zero=False, dtype=None):
    """NDHWC activation in `like`'s dtype (fp32, or bf16 on the mixed-precision path) unless `dtype` says otherwise."""
    dt = dtype if dtype is not None else (like.dtype if like.dtype == torch.bfloat16 else torch.float32)
    t = torch.empty((N, Cc, D, H, W), dtype=dt, device=like.device, memory_format=torch.channels_last_3d)
    return t.zero_() if zero else t


# ---- weight forms kept across launches ----------------------------------------------------------------------------
# A convolution needs its weights as a kernel panel (pack_weights) and, on the fp32 Winograd kernels, as
# transform-domain fragments (the library's weight-transform launch into `wino_ws`): two 5-20 us launches in front of
# every forward and every input-gradient kernel.  Both depend on the parameter's VALUES and the layer geometry only.
# For weights that take no gradient in the pass at hand -- frozen parameters, passes under torch.no_grad(): the joint
# step's teacher, the tiled predictor walking hundreds of tiles, validation -- they are kept per (parameter, geometry)
# and rebuilt, where they are needed, when the
# parameter has changed: its version counter has moved (load_state_dict, any in-place torch op) or an optimizer has
# stepped over it (torch's fused optimizers do NOT move version counters, so a global optimizer-step post hook stamps
# the parameters of every optimizer that steps).  A write through `.data` is seen by neither, by torch's design: call
# invalidate_weight_forms() after one.
# Trainable parameters in a recorded pass are NOT kept: every form would be stale once per step anyway.  Rebuilding all
# stale forms of a step in one batch in front of the first convolution (on one side stream next to the forward, or
# fanned out over 2 / 4 / 8 streams and joined) was measured and is SLOWER than the launches where they stand
# (profiles/r03_ab_weight_forms.txt: cfg-2 +0.4..0.6 ms, cfg-3 +0.6..1.0 ms): in line, each small launch runs in the
# shadow of the matrix-core kernels around it, whose clocks the power budget sets -- the 1.5 ms these launches sum to in
# a kernel trace is not on the step's critical path.
WEIGHT_FORM_CACHE = True     # False: every call packs / transforms for itself (tests compare the two)


def _after_optimizer_step(opt, args, kwargs):
    for g in opt.param_groups:
        for p in g["params"]:
            p._rehr_stamp = getattr(p, "_rehr_stamp", 0) + 1


_register_step_hook(_after_optimizer_step)


def _ver(p):
    """What a form remembers of the parameter it was made from."""
    return (p._version, getattr(p, "_rehr_stamp", 0))


keep_forms = False           # set by ops.fused_conv3d / _FusedConv.backward in front of every launch sequence: the weight of this node takes
                             # no gradient in this pass (frozen parameter, or nothing is being recorded)


def _keeps_forms(w):
    return WEIGHT_FORM_CACHE and keep_forms and isinstance(w, torch.nn.Parameter)


class _Form:
    __slots__ = ("param", "version", "out", "make", "stream", "readers", "dep", "__weakref__")

    def __init__(self, key, param, make, dep=None):
        self.param = weakref.ref(param, lambda _r, k=key: _drop_form(k))   # the forms go when the parameter goes
        self.version = None          # _ver(parameter) `out` was made from
        self.out = None              # pack: the panel tensor; Winograd: list of scratch tensors (one per descriptor)
        self.make = make             # make(parameter): launches the rebuild on the current stream
        self.stream = None           # the stream of the last rebuild
        self.readers = set()         # streams that have consumed `out` since (a rebuild has to wait for them)
        self.dep = dep               # Winograd forms: the pack form they read


_forms = {}                # key -> _Form
_form_of_panel = {}        # id(panel tensor) -> pack form (Winograd forms find the parameter behind a `wp`)
form_rebuilds = 0          # launches issued for (re)building kept forms (tests look at this)


def _drop_form(key):
    f = _forms.pop(key, None)
    if f is not None and key[0] == "pack":
        _form_of_panel.pop(id(f.out), None)


def invalidate_weight_forms():
    """Forget every kept weight form (after writing parameters through `.data`, which no version counter sees)."""
    _forms.clear()
    _form_of_panel.clear()


def _form_ready(f, p):
    """Make form `f` of parameter `p` current and order the current stream behind its last rebuild."""
    global form_rebuilds
    cur = torch.cuda.current_stream(p.device)
    v = _ver(p)
    if f.version != v:
        if f.dep is not None:
            _form_ready(f.dep, p)
        for r in f.readers:                             # nobody may still be reading what is overwritten
            if r != cur:
                cur.wait_stream(r)
        if f.stream is not None and f.stream != cur:
            cur.wait_stream(f.stream)
        f.make(p)
        form_rebuilds += 1
        f.version, f.stream, f.readers = v, cur, set()
    if f.stream != cur and cur not in f.readers:        # made on another stream: once per rebuild and consumer stream
        cur.wait_stream(f.stream)
    f.readers.add(cur)


def _pack_launch(src, out, A, Apad, B, T, transpose):
    if out.dtype == torch.bfloat16:
        L.check(L.load().rehr_pack_weights_bf16(_ptr(src), _ptr(out), A, Apad, B, T, int(transpose), _stream()),
                "rehr_pack_weights_bf16")
    else:
        L.check(L.load().rehr_pack_weights_f32(_ptr(src), _ptr(out), A, Apad, B, T, int(transpose), _stream()),
                "rehr_pack_weights_f32")


def pack_weights(w, A, Apad, B, T, transpose, dtype=torch.float32, part=None):
    """fp32 master weights in the torch parameter layout -> kernel panel [T][Apad][B] in `dtype` (fp32 / bf16).
    `part` = (dim, lo, count): the panel of w.narrow(dim, lo, count) (the halves of a virtual channel concat).
    Panels of frozen parameters / of no-grad passes are kept until the parameter changes ("weight forms" above)."""
    _chk_dev(w)
    if w.dtype != torch.float32:
        raise L.RehrsegHipError("master weights are float32")

    def src(p):
        return (p if part is None else p.narrow(*part)).contiguous()

    if not _keeps_forms(w):
        out = torch.empty((T, Apad, B), dtype=dtype, device=w.device)
        _pack_launch(src(w), out, A, Apad, B, T, transpose)
        return out
    key = ("pack", id(w), tuple(w.shape), part, A, Apad, B, T, bool(transpose), dtype)
    f = _forms.get(key)
    if f is None or f.param() is not w:
        out = torch.empty((T, Apad, B), dtype=dtype, device=w.device)
        f = _forms[key] = _Form(key, w, lambda p: _pack_launch(src(p), out, A, Apad, B, T, transpose))
        f.out = out
        _form_of_panel[id(out)] = f
    _form_ready(f, w)
    return f.out


# Trainable weights in a recorded pass (forms not kept): the fp32 Winograd kernels read only the transform-domain
# fragments, so the panel would be written to be read once.  ops._pack gets a _LazyPanel for them; gather_gemm /
# gather_gemm_multi fill the scratch of the call straight from the parameter (rehr_gather_gemm_wino_forms_f32: one pass,
# the halves of a virtual concat read in place) and launch with REHR_GG_WS_READY.  The panel is packed only when the
# library says that the launch would not run a Winograd kernel for every part (REHR_ENOSUP: the same decision as the
# launch's, joint plans of the parts and the fused transposed-convolution kernel included) or no scratch is wanted.
USE_ONEPASS_FORMS = True     # False: pack, then transform (tests and the A/B compare the two; the bits are the same)
onepass_form_calls = 0       # calls whose forms came straight from the parameter (tests look at this)


class _LazyPanel:
    """The arguments of pack_weights for a parameter whose panel may never be needed."""
    __slots__ = ("w", "A", "Apad", "B", "T", "transpose", "part", "_out")

    def __init__(self, w, A, Apad, B, T, transpose, part):
        self.w, self.A, self.Apad, self.B, self.T, self.transpose, self.part = w, A, Apad, B, T, bool(transpose), part
        self._out = None

    def panel(self):
        if self._out is None:
            self._out = pack_weights(self.w, self.A, self.Apad, self.B, self.T, self.transpose, part=self.part)
        return self._out


def lazy_weights(w, A, Apad, B, T, transpose, part=None):
    """pack_weights for the fp32 gather-GEMM calls of ops: the panel itself, or -- for weights whose forms are not
    kept -- a _LazyPanel that gather_gemm / gather_gemm_multi resolve."""
    _chk_dev(w)
    if (not USE_ONEPASS_FORMS or not USE_WINOGRAD or _keeps_forms(w) or w.dtype != torch.float32 or w.dim() != 5 or
            not w.is_contiguous()):
        return pack_weights(w, A, Apad, B, T, transpose, part=part)
    return _LazyPanel(w, A, Apad, B, T, transpose, part)


def _onepass_forms(arr, n, needs, lazy):
    """Scratch for every descriptor of the call, filled from the parameter.  Returns (what must stay referenced, True)
    when the call can run with REHR_GG_WS_READY; (the same, False) when the library wants the panel -- the scratch stays
    attached for the transforms of the launch; None when some descriptor wants no scratch (nothing attached)."""
    global onepass_form_calls
    if not all(needs) or any(arr[i].Cout != lazy.A or arr[i].Cin != lazy.B for i in range(n)):
        return None
    w = lazy.w
    keep = _attach_ws(arr, n, needs, None, w)       # (w is no kept panel: fresh scratch, counted as a Winograd launch)
    dest_dim = 1 if lazy.transpose else 0
    dest_lo = src_lo = 0
    if lazy.part is not None:
        if lazy.part[0] == dest_dim:
            dest_lo = lazy.part[1]
        else:
            src_lo = lazy.part[1]
    rc = L.load().rehr_gather_gemm_wino_forms_f32(arr, n, _ptr(w), w.shape[0], w.shape[1], lazy.T, dest_dim, dest_lo,
                                                  src_lo, _stream())
    if rc == -2:                                    # REHR_ENOSUP: some part needs the panel
        return keep, False
    L.check(rc, "rehr_gather_gemm_wino_forms_f32")
    for i in range(n):
        arr[i].flags |= L.GG_WS_READY
    onepass_form_calls += 1
    return keep, True


# Kernel selection travels in the descriptors (the library reads no environment).  With `flags` / `debug_flags` = 0
# the library picks its measured-best kernels: forward / input gradient take the Winograd kernels when the descriptor
# carries scratch.  The switches below set `debug_flags` bits (unstable, include/rehrseg_hip.h): tests flip them to
# compare kernel organisations with each other (transform-domain against direct, brick against per-tap, ...).
USE_WINOGRAD = True
USE_WINOGRAD_WGRAD = True   # False -> REHR_DBG_WGRAD_DIRECT
USE_HALO_BF16 = True   # mixed precision: LDS halo-brick kernel for unit-stride 3x3(x3) taps (False -> REHR_DBG_GG_NO_HALO)
WGRAD_TAP_COLOCATE = True   # Winograd weight gradient: the depth taps of a split on one XCD (shared dY / x in L2)
USE_WGRAD_TAP_SKIP = True   # Winograd weight gradient: a depth tap walks only the slices whose source slice exists
W32P_BLOCKS = 0   # 0: the library picks; 1 / 2 force two 256-thread blocks per CU / one 512-thread block (tests, A/B)
PHASE_INTERLEAVE = False   # multi-phase launches: the phases of a lattice tile as consecutive blocks of one XCD (measured slower)
WINO_BAND_MAJOR = True   # fp32 Winograd tile order: an XCD walks depth inside a band of rows (L2 reuse of the depth taps)
USE_TCONV_KS = True   # kernel == stride transposed convolutions: all phases of an input tile in one block (tconv_ks.hip)
USE_WINO_FLAT8 = True   # fp32 Winograd on planes that 16 x 16 regions tile badly: wino_flat8_conv_kernel
WINO_FLAT8_TILES = 0    # 0: the library picks 32 or 64 tiles per block; 1 / 2 force 32 / 64 (tests, A/B)
wino_wgrad_launches = 0  # weight gradients taken by the Winograd kernel
wino_launches = 0  # contractions handed to the Winograd kernels so far (tests look at this)


def _gg_desc(d, x1, x2, c1, src_dims, Cin, lattice, s, b, taps, KH, KW, wp, Npad, y, y_dims, Cout,
             os_, ob, bias, act, slope, stats, stats_mode, tile):
    _chk_dev(x1, x2, wp, y, bias, f64=(stats,))
    d.x1, d.x2, d.c1 = _ptr(x1), _ptr(x2), c1
    d.ldx1 = x1.shape[1]
    d.ldx2 = x2.shape[1] if x2 is not None else 0
    d.N = x1.shape[0]
    d.Di, d.Hi, d.Wi = src_dims
    d.Cin = Cin
    d.Ld, d.Lh, d.Lw = lattice
    d.sd, d.sh, d.sw = s
    d.bd, d.bh, d.bw = b
    d.td, d.th, d.tw = _taps(taps[0]), _taps(taps[1]), _taps(taps[2])
    d.KH, d.KW = KH, KW
    d.wp, d.Npad = _ptr(wp), Npad
    d.y = _ptr(y)
    d.Dy, d.Hy, d.Wy = y_dims
    d.Cout, d.ldy = Cout, y.shape[1]
    d.osd, d.osh, d.osw = os_
    d.obd, d.obh, d.obw = ob
    d.bias, d.act, d.slope = _ptr(bias), act, slope
    d.stats, d.stats_mode = _ptr(stats), stats_mode
    d.tile_d, d.tile_h, d.tile_w = tile
    d.wino_ws, d.wino_ws_bytes = None, 0
    d.flags = 0
    d.debug_flags = 0
    need = 0
    if x1.dtype == torch.bfloat16:
        if wp.dtype != torch.bfloat16 or (x2 is not None and x2.dtype != torch.bfloat16):
            raise L.RehrsegHipError("mixed-precision gather-GEMM: x1, x2 and the packed weights must all be bfloat16")
        if bias is not None and bias.dtype != torch.float32:
            raise L.RehrsegHipError("bias stays float32")
        d.flags = L.GG_Y_F32 if y.dtype == torch.float32 else 0
        d.debug_flags = (0 if USE_HALO_BF16 else L.DBG_GG_NO_HALO)
    elif wp.dtype != torch.float32 or y.dtype != torch.float32 or (x2 is not None and x2.dtype != torch.float32):
        raise L.RehrsegHipError("fp32 gather-GEMM: every operand must be float32")
    elif USE_WINOGRAD and tile[0] >= 0:
        d.debug_flags = ((0 if USE_WINO_FLAT8 else L.DBG_GG_NO_FLAT8) |
                         {1: L.DBG_GG_W32P_TWO_PER_CU, 2: L.DBG_GG_W32P_ONE_PER_CU}.get(W32P_BLOCKS, 0) |
                         {1: L.DBG_GG_FLAT8_HALF, 2: L.DBG_GG_FLAT8_FULL}.get(WINO_FLAT8_TILES, 0))
        need = L.load().rehr_gather_gemm_wino_bytes(C.byref(d))
    if PHASE_INTERLEAVE:
        d.debug_flags |= L.DBG_GG_INTERLEAVE
    if not USE_TCONV_KS:
        d.debug_flags |= L.DBG_GG_NO_TCONV_KS
    if not WINO_BAND_MAJOR:
        d.debug_flags |= L.DBG_GG_SLICE_MAJOR
    # (the Winograd scratch is attached by _attach_ws once every descriptor of the call is known)
    _gg_desc.need = need
    _gg_desc.sig = (c1, x1.shape[1], x2.shape[1] if x2 is not None else 0, x1.shape[0], tuple(src_dims), Cin,
                    tuple(lattice), tuple(s), tuple(b), tuple(tuple(t) for t in taps), KH, KW, Npad, tuple(y_dims), Cout,
                    y.shape[1], tuple(os_), tuple(ob), bias is not None, act, stats_mode, tuple(tile), d.debug_flags)
    return _algo_flops(d.N, lattice, s, b, taps, src_dims, Cin, Cout) if _prof is not None else 0.0


def _attach_ws(descs, n, needs, sigs, wp):
    """Winograd scratch for the descriptors of one call that want it.  Returns what must stay referenced until the
    launch has been enqueued.  When `wp` is the kept panel of a parameter the transformed weights are kept too (one form
    per call geometry) and the call runs with REHR_GG_WS_READY."""
    if not any(needs):
        return None
    global wino_launches
    wino_launches += sum(1 for nb in needs if nb)
    dev = wp.device
    pf = _form_of_panel.get(id(wp)) if WEIGHT_FORM_CACHE else None
    p = pf.param() if pf is not None else None
    if p is None or not _keeps_forms(p):
        keeps = [torch.empty(nb // 4, dtype=torch.float32, device=dev) if nb else None for nb in needs]
        for i in range(n):
            if needs[i]:
                descs[i].wino_ws, descs[i].wino_ws_bytes = _ptr(keeps[i]), needs[i]
        return keeps
    key = ("ws", id(p), id(pf), tuple(sigs))
    f = _forms.get(key)
    if f is None or f.param() is not p or f.dep is not pf:
        outs = [torch.empty(nb // 4, dtype=torch.float32, device=dev) if nb else None for nb in needs]
        cp = (L.GatherGemmDesc * n)()       # the rebuild call: the same descriptors, transforms only (operand pointers
        for i in range(n):                  # other than wp / wino_ws go stale and are not dereferenced)
            C.memmove(C.byref(cp[i]), C.byref(descs[i]), C.sizeof(L.GatherGemmDesc))
            if needs[i]:
                cp[i].wino_ws, cp[i].wino_ws_bytes = _ptr(outs[i]), needs[i]
            cp[i].flags |= L.GG_WS_ONLY

        def make(_p, cp=cp, n=n):
            L.check(L.load().rehr_gather_gemm_multi_f32(cp, n, _stream()), "rehr_gather_gemm_multi_f32 (weight forms)")

        f = _forms[key] = _Form(key, p, make, dep=pf)
        f.out = outs
    _form_ready(f, p)
    for i in range(n):
        if needs[i]:
            descs[i].wino_ws, descs[i].wino_ws_bytes = _ptr(f.out[i]), needs[i]
        descs[i].flags |= L.GG_WS_READY
    return f.out


def _lazy_ws(arr, n, needs, lazy):
    """The scratch of a call whose weights came as a _LazyPanel: forms straight from the parameter where every part
    runs a Winograd kernel, else the panel (packed now) and the transforms of the launch."""
    got = _onepass_forms(arr, n, needs, lazy)
    if got is not None and got[1]:
        return got[0]
    panel = lazy.panel()
    _set_panel(arr, n, panel)
    keep = got[0] if got is not None else _attach_ws(arr, n, needs, None, panel)
    return (keep, panel)


def _gg_tag(arr, n=1, bf16=False):
    """Shape of the call and, in brackets, the kernel the library runs for it: the Winograd route of a descriptor that
    carries scratch, else the direct kernel(s) of the parts.  Evaluated by _timed only while a profile is running."""
    d = arr[0]
    name = _ROUTE_NAMES.get(wino_route(d)[0]) if d.wino_ws else None
    if name is None:
        try:
            kinds = [_DIRECT_NAMES[bf16].get(r, "none") for r in direct_route(arr, n, bf16)]
            name = "+".join(sorted(set(kinds), key=kinds.index))     # each kernel once, in part order
        except L.RehrsegHipError:                                    # (the launch has raised the same error already)
            name = "invalid"
    return (f"N{d.N} {d.Cin}->{d.Cout} lattice {d.Ld}x{d.Lh}x{d.Lw} stride {d.sd}{d.sh}{d.sw} "
            f"taps {d.td.count}x{d.th.count}x{d.tw.count}" + (" +x2" if d.x2 else "") + f" [{name}]")


_ROUTE_NAMES = {L.GG_ROUTE_FLAT8: "flat8", L.GG_ROUTE_W32P: "w32p", L.GG_ROUTE_BIG8: "big8", L.GG_ROUTE_SMALL: "small",
                L.GG_ROUTE_FLAT22: "flat22", L.GG_ROUTE_REGION22: "region22"}
# (kind, variant) of rehr_gather_gemm_direct_route -> kernel name, fp32 / bf16
_DIRECT_NAMES = {False: {(L.GG_DIRECT_GENERIC, 0): "generic", (L.GG_DIRECT_TCONV_KS, 0): "tconv_ks",
                         (L.GG_DIRECT_HALO, 1): "halo bn64", (L.GG_DIRECT_HALO, 2): "halo bn32"},
                 True: {(L.GG_DIRECT_GENERIC, 0): "generic", (L.GG_DIRECT_TCONV_KS, 0): "tconv_ks",
                        (L.GG_DIRECT_HALO, 1): "halo 4x8x16", (L.GG_DIRECT_HALO, 2): "halo 8x8x8",
                        (L.GG_DIRECT_HALO, 3): "halo 2x16x16"}}


def direct_route(descs, count, bf16):
    """[(kind, variant)] per part of rehr_gather_gemm_direct_route: the direct kernel (L.GG_DIRECT_*) that a call of the
    fp32 / bf16 multi entry point with these `count` descriptors runs for each part no Winograd kernel takes."""
    out = (C.c_int32 * count)()
    L.check(L.load().rehr_gather_gemm_direct_route(descs, count, int(bool(bf16)), out), "rehr_gather_gemm_direct_route")
    return [(r & 255, (r >> 8) & 255) for r in out]


def wino_route(d):
    """(route, variant) of rehr_gather_gemm_wino_route: which fp32 Winograd kernel the library runs for this descriptor
    when its scratch is attached (L.GG_ROUTE_*; 0 = none), and the kernel's variant."""
    r = int(L.load().rehr_gather_gemm_wino_route(C.byref(d)))
    return r & 255, (r >> 8) & 255


def _gg_family(d):
    """Profiling family of a launch: the library says which kernel takes the descriptor (no guess from the tap counts).
    The families stay the two transforms whose issue rates bench.py prices."""
    if _prof is None:
        return None             # no profile is running: _timed drops the family, so the library is not asked
    if not d.wino_ws:
        return "gather_gemm"
    route = wino_route(d)[0]
    if route == L.GG_ROUTE_NONE:
        return "gather_gemm"
    return "wino22_conv" if route in (L.GG_ROUTE_FLAT22, L.GG_ROUTE_REGION22) else "wino_conv"


def _with_wp(args, wp):
    return args[:11] + (wp,) + args[12:]


def _set_panel(arr, n, panel):
    for i in range(n):
        arr[i].wp = _ptr(panel)


def gather_gemm(*args):
    lazy = args[11] if isinstance(args[11], _LazyPanel) else None
    if lazy is not None:
        # the descriptor is planned with the parameter standing in for the panel (wp only has to pass the validation;
        # a parameter that is not 16-byte aligned gets no Winograd scratch and takes the panel path below)
        args = _with_wp(args, lazy.w)
    d = L.GatherGemmDesc()
    flops = _gg_desc(d, *args)
    if args[0].dtype == torch.bfloat16:
        with _timed("gather_gemm_bf16", flops, lambda: _gg_tag((L.GatherGemmDesc * 1)(d), bf16=True)):
            L.check(L.load().rehr_gather_gemm_bf16(C.byref(d), _stream()), "rehr_gather_gemm_bf16")
        return
    arr = (L.GatherGemmDesc * 1)(d)
    keep = _lazy_ws(arr, 1, [_gg_desc.need], lazy) if lazy is not None else \
        _attach_ws(arr, 1, [_gg_desc.need], [_gg_desc.sig], args[11])
    with _timed(_gg_family(arr[0]), flops, lambda: _gg_tag(arr)):
        L.check(L.load().rehr_gather_gemm_multi_f32(arr, 1, _stream()), "rehr_gather_gemm_f32")
    del keep


def gather_gemm_multi(calls):
    """`calls` = argument tuples of gather_gemm for the stride phases of one layer: one grid."""
    if len(calls) == 1:
        return gather_gemm(*calls[0])
    lazy = calls[0][11] if isinstance(calls[0][11], _LazyPanel) else None
    if lazy is not None:
        calls = [_with_wp(a, lazy.w) for a in calls]      # (the parameter stands in for the panel: see gather_gemm)
    arr = (L.GatherGemmDesc * len(calls))()
    flops, needs, sigs = 0.0, [], []
    for i, a in enumerate(calls):
        flops += _gg_desc(arr[i], *a)
        needs.append(_gg_desc.need)
        sigs.append(_gg_desc.sig)
    if calls[0][0].dtype == torch.bfloat16:
        with _timed("gather_gemm_bf16", flops, lambda: f"{len(calls)} parts of " + _gg_tag(arr, len(calls), bf16=True)):
            L.check(L.load().rehr_gather_gemm_multi_bf16(arr, len(calls), _stream()), "rehr_gather_gemm_multi_bf16")
        return
    keep = _lazy_ws(arr, len(calls), needs, lazy) if lazy is not None else \
        _attach_ws(arr, len(calls), needs, sigs, calls[0][11])   # every part its own scratch: ONE launch runs them all
    with _timed(_gg_family(arr[0]) if all(arr[i].wino_ws for i in range(len(calls))) else "gather_gemm", flops,
                lambda: f"{len(calls)} parts of " + _gg_tag(arr, len(calls))):
        L.check(L.load().rehr_gather_gemm_multi_f32(arr, len(calls), _stream()), "rehr_gather_gemm_multi_f32")
    del keep


def sum_slabs_bias_act(slabs, S, bias, act, slope, stats=None, out_dtype=None):
    """slabs: (S*N, C, D, H, W) NDHWC fp32 partial results -> (N, C, D, H, W) = act(bias + sum over S) in `out_dtype`
    (fp32, or bf16 on the mixed-precision path); `stats` (N, C, 2) double, pre-zeroed: also accumulate the per-(n,c)
    sum / sum of squares (of the fp32 sums)."""
    _chk_dev(slabs, bias, f64=(stats,))
    if slabs.dtype != torch.float32:
        raise L.RehrsegHipError("split-K slabs are float32")
    SN, Cc, D, H, W = slabs.shape
    N = SN // S
    bf = out_dtype == torch.bfloat16
    y = new_act(N, Cc, D, H, W, like=slabs, dtype=torch.bfloat16 if bf else torch.float32)
    rows = N * D * H * W
    lib = L.load()
    if stats is not None:
        fn = lib.rehr_sum_slabs_stats_bf16 if bf else lib.rehr_sum_slabs_stats_f32
        L.check(fn(_ptr(slabs), S, rows * Cc, _ptr(bias), _ptr(y), N, D * H * W, Cc, act, slope, _ptr(stats), _stream()),
                "rehr_sum_slabs_stats")
        return y
    fn = lib.rehr_sum_slabs_bias_act_bf16 if bf else lib.rehr_sum_slabs_bias_act_f32
    L.check(fn(_ptr(slabs), S, rows * Cc, _ptr(bias), _ptr(y), rows, Cc, act, slope, _stream()), "rehr_sum_slabs_bias_act")
    return y


def wgrad(l, Ca, g, Cg, N, lattice, g_dims, s, b, taps, KH, KW, dst, dst_off, dst_strides, accumulate, dbias):
    """dst (fp32, the master-weight gradient) from l / g in fp32, or both in bf16 (mixed precision: no dbias)."""
    _chk_dev(l, g, dst, dbias)
    bf16 = l.dtype == torch.bfloat16
    if (g.dtype == torch.bfloat16) != bf16 or dst.dtype != torch.float32:
        raise L.RehrsegHipError("weight gradient: l and g share one dtype (fp32 or bf16), dst is float32")
    d = L.WgradDesc()
    d.l, d.ldl, d.Ca = _ptr(l), l.shape[1], Ca
    d.g, d.ldg, d.Cg = _ptr(g), g.shape[1], Cg
    d.N = N
    d.Ld, d.Lh, d.Lw = lattice
    d.Dg, d.Hg, d.Wg = g_dims
    d.sd, d.sh, d.sw = s
    d.bd, d.bh, d.bw = b
    d.td, d.th, d.tw = _taps(taps[0]), _taps(taps[1]), _taps(taps[2])
    d.KH, d.KW = KH, KW
    d.dst = C.c_void_p(dst.data_ptr() + 4 * dst_off)
    d.dst_sa, d.dst_sc, d.dst_st = dst_strides
    d.accumulate = int(accumulate)
    d.dbias = _ptr(dbias)
    d.flags = 0
    d.debug_flags = ((0 if USE_WINOGRAD_WGRAD else L.DBG_WGRAD_DIRECT) | (0 if USE_WGRAD_TAP_SKIP else L.DBG_WGRAD_NO_TAP_SKIP) |
                     (0 if WGRAD_TAP_COLOCATE else L.DBG_WGRAD_NO_TAP_COLOCATE))
    lib = L.load()
    flops = _algo_flops(N, lattice, s, b, taps, g_dims, Ca, Cg) if _prof is not None else 0.0
    if bf16:
        if dbias is not None:
            raise L.RehrsegHipError("mixed-precision weight gradient has no fused bias gradient (use channel_sum)")
        ws = _workspace(lib.rehr_wgrad_bf16_workspace_bytes, (C.byref(d),), l.device, "rehr_wgrad_bf16_workspace_bytes")
        d.workspace, d.workspace_bytes = _ptr(ws), ws.numel()
        with _timed("wgrad_bf16", flops, lambda: f"N{N} {Ca}x{Cg} lattice {tuple(lattice)} stride {tuple(s)} "
                                             f"taps {taps[0][0]}x{taps[1][0]}x{taps[2][0]}"):
            L.check(lib.rehr_wgrad_bf16(C.byref(d), _stream()), "rehr_wgrad_bf16")
        return
    ws = _workspace(lib.rehr_wgrad_workspace_bytes, (C.byref(d),), l.device, "rehr_wgrad_workspace_bytes")
    global wino_wgrad_launches
    wino = int(lib.rehr_wgrad_uses_winograd(C.byref(d)))
    wino_wgrad_launches += wino
    d.workspace, d.workspace_bytes = _ptr(ws), ws.numel()
    with _timed(("wino_wgrad" if d.th.count == 3 else "wino22_wgrad") if wino else "wgrad", flops,
                lambda: f"N{N} {Ca}x{Cg} lattice {tuple(lattice)} stride {tuple(s)} taps {taps[0][0]}x{taps[1][0]}x{taps[2][0]}"):
        L.check(lib.rehr_wgrad_f32(C.byref(d), _stream()), "rehr_wgrad_f32")


def _direct_desc(x, w, bias, y, stride, pad, act, slope, stats, stats_mode):
    d = L.DirectConvDesc()
    N, Cin, Di, Hi, Wi = x.shape
    Cout, _, KD, KH, KW = w.shape
    _, _, Do, Ho, Wo = y.shape
    d.x, d.ldx, d.N, d.Di, d.Hi, d.Wi, d.Cin = _ptr(x), Cin, N, Di, Hi, Wi, Cin
    d.w, d.bias = _ptr(w), _ptr(bias)
    d.y, d.ldy, d.Do, d.Ho, d.Wo, d.Cout = _ptr(y), Cout, Do, Ho, Wo, Cout
    d.KD, d.KH, d.KW = KD, KH, KW
    d.sd, d.sh, d.sw = stride
    d.pd, d.ph, d.pw = pad
    d.act, d.slope = act, slope
    d.stats, d.stats_mode = _ptr(stats), stats_mode
    return d


def _shape_desc(x_shape, w_shape, stride, pad):
    """A descriptor without pointers, for the library's questions about a shape: dense NDHWC tensors, the output extent
    the convolution gives."""
    d = L.DirectConvDesc()
    d.N, d.Cin, d.Di, d.Hi, d.Wi = x_shape
    d.Cout, _, d.KD, d.KH, d.KW = w_shape
    d.ldx, d.ldy = d.Cin, d.Cout
    d.sd, d.sh, d.sw = stride
    d.pd, d.ph, d.pw = pad
    d.Do, d.Ho, d.Wo = ((i + 2 * p - k) // s + 1 for i, k, s, p in zip(x_shape[2:], w_shape[2:], stride, pad))
    return d


@functools.lru_cache(maxsize=None)
def small_cin_bf16_out_ok(x_shape, w_shape, stride, pad):
    """Shapes whose thin-input forward runs on the matrix cores (thin_cin_conv.hip) and can therefore store bf16."""
    return bool(L.load().rehr_conv_small_cin_fwd_on_mfma(C.byref(_shape_desc(x_shape, w_shape, stride, pad))))


def small_cin_fwd(x, w, bias, y, stride, pad, act, slope, stats, stats_mode):
    """x, w, bias fp32; y fp32, or bf16 on the mixed-precision path (matrix-core shapes only)."""
    _chk_dev(x, w, bias, y, f64=(stats,))
    if x.dtype != torch.float32:
        raise L.RehrsegHipError("thin-input conv: the input stays float32")
    d = _direct_desc(x, w.contiguous(), bias, y, stride, pad, act, slope, stats, stats_mode)
    if y.dtype == torch.bfloat16:
        L.check(L.load().rehr_conv_small_cin_fwd_ybf16(C.byref(d), _stream()), "rehr_conv_small_cin_fwd_ybf16")
        return
    L.check(L.load().rehr_conv_small_cin_fwd_f32(C.byref(d), _stream()), "rehr_conv_small_cin_fwd_f32")


def im2col(x, w, out_dims, stride, pad, Kpad):
    """(N, Kpad, Do, Ho, Wo) NDHWC columns of a thin-input conv (k = ci*T + tap)."""
    _chk_dev(x, w)
    N = x.shape[0]
    col = new_act(N, Kpad, *out_dims, like=x)
    d = _direct_desc(x, w, None, col, stride, pad, 0, 0.0, None, 0)
    d.Cout, d.ldy = w.shape[0], Kpad
    L.check(L.load().rehr_im2col_f32(C.byref(d), _ptr(col), Kpad, _stream()), "rehr_im2col_f32")
    return col


def small_cin_wgrad_on_mfma(x, w, dy, stride, pad):
    """True when the thin-input weight gradient has its own matrix-core kernel for this shape (no im2col route)."""
    d = _direct_desc(x, w.contiguous(), None, dy, stride, pad, 0, 0.0, None, 0)
    return bool(L.load().rehr_conv_small_cin_wgrad_on_mfma(C.byref(d)))


def small_cin_wgrad(x, w, dy, stride, pad, want_bias):
    """dy fp32, or bf16 (mixed precision) where the matrix-core kernel takes the shape (else cast up first)."""
    _chk_dev(x, w, dy)
    lib = L.load()
    d = _direct_desc(x, w.contiguous(), None, dy, stride, pad, 0, 0.0, None, 0)
    if dy.dtype == torch.bfloat16 and not lib.rehr_conv_small_cin_wgrad_on_mfma(C.byref(d)):
        dy = dy.float()
        d.y = _ptr(dy)
    ws = _workspace(lib.rehr_conv_small_cin_wgrad_workspace_bytes, (C.byref(d),), x.device,
                    "rehr_conv_small_cin_wgrad_workspace_bytes")
    dw = torch.empty_like(w, memory_format=torch.contiguous_format)
    db = torch.empty(w.shape[0], dtype=torch.float32, device=x.device) if want_bias else None
    fn = lib.rehr_conv_small_cin_wgrad_dybf16 if dy.dtype == torch.bfloat16 else lib.rehr_conv_small_cin_wgrad_f32
    L.check(fn(C.byref(d), _ptr(dw), _ptr(db), _ptr(ws), ws.numel(), _stream()), "rehr_conv_small_cin_wgrad")
    return dw, db


def small_cout_fwd(x, w, bias, y, pad, act, slope):
    _chk_dev(x, w, bias, y)
    d = _direct_desc(x, w.contiguous(), bias, y, (1, 1, 1), pad, act, slope, None, 0)
    L.check(L.load().rehr_conv_small_cout_fwd_f32(C.byref(d), _stream()), "rehr_conv_small_cout_fwd_f32")


def small_cout_dgrad(dy, w, x_shape, pad):
    _chk_dev(dy, w)
    dx = new_act(*x_shape, like=dy)
    d = _direct_desc(dx, w.contiguous(), None, dy, (1, 1, 1), pad, 0, 0.0, None, 0)
    L.check(L.load().rehr_conv_small_cout_dgrad_f32(C.byref(d), _ptr(dx), _stream()),
            "rehr_conv_small_cout_dgrad_f32")
    return dx


def small_cout_wgrad(x, w, dy, pad, want_bias):
    _chk_dev(x, w, dy)
    d = _direct_desc(x, w.contiguous(), None, dy, (1, 1, 1), pad, 0, 0.0, None, 0)
    lib = L.load()
    ws = _workspace(lib.rehr_conv_small_cout_wgrad_workspace_bytes, (C.byref(d),), x.device,
                    "rehr_conv_small_cout_wgrad_workspace_bytes")
    dw = torch.empty_like(w, memory_format=torch.contiguous_format)
    db = torch.empty(w.shape[0], dtype=torch.float32, device=x.device) if want_bias else None
    L.check(lib.rehr_conv_small_cout_wgrad_f32(C.byref(d), _ptr(dw), _ptr(db), _ptr(ws), ws.numel(), _stream()),
            "rehr_conv_small_cout_wgrad_f32")
    return dw, db


def se_gate_fwd(stats, w, b, N, Cc, S):
    _chk_dev(w, b, f64=(stats,))
    gate = torch.empty((N, Cc), dtype=torch.float32, device=stats.device)
    mean = torch.empty((N, Cc), dtype=torch.float32, device=stats.device)
    L.check(L.load().rehr_se_gate_fwd_f32(_ptr(stats), _ptr(w.contiguous()), _ptr(b.contiguous()), _ptr(gate),
                                          _ptr(mean), N, Cc, S, _stream()), "rehr_se_gate_fwd_f32")
    return gate, mean


def _nsc(x):
    N, Cc, D, H, W = x.shape
    return N, D * H * W, Cc


def scale_res_act_fwd(x, gate, res, act, slope):
    _chk_dev(x, gate, res)
    _same_dtype(x, res)
    N, S, Cc = _nsc(x)
    y = new_act(*x.shape, like=x)
    fn, name = _fn("rehr_scale_res_act_fwd", x)
    L.check(fn(_ptr(x), Cc, _ptr(gate), _ptr(res), Cc, _ptr(y), Cc, N, S, Cc, act, slope, _stream()), name)
    return y


def scale_res_act_bwd(dy, y, x, gate, want_dres, act, slope):
    _chk_dev(dy, y, x, gate)
    _same_dtype(dy, y, x)
    N, S, Cc = _nsc(x)
    dx = new_act(*x.shape, like=x)
    dres = new_act(*x.shape, like=x) if want_dres else None
    dgate = zeros_f64((N, Cc), x.device)
    fn, name = _fn("rehr_scale_res_act_bwd", x)
    L.check(fn(_ptr(dy), Cc, _ptr(y), Cc, _ptr(x), Cc, _ptr(gate), _ptr(dx), Cc, _ptr(dres), Cc, _ptr(dgate), N, S, Cc,
               act, slope, _stream()), name)
    return dx, dres, dgate


def se_gate_bwd(dgate, gate, mean, w, S):
    _chk_dev(gate, mean, w, f64=(dgate,))
    N, Cc = gate.shape
    dw = torch.empty((Cc, Cc), dtype=torch.float32, device=gate.device)
    db = torch.empty((Cc,), dtype=torch.float32, device=gate.device)
    k = torch.empty((N, Cc), dtype=torch.float32, device=gate.device)
    L.check(L.load().rehr_se_gate_bwd_f32(_ptr(dgate), _ptr(gate), _ptr(mean), _ptr(w.contiguous()), _ptr(dw),
                                          _ptr(db), _ptr(k), N, Cc, S, _stream()), "rehr_se_gate_bwd_f32")
    return dw, db, k


def add_channel_const(x, k):
    _chk_dev(x, k)
    N, S, Cc = _nsc(x)
    fn, name = _fn("rehr_add_channel_const", x)
    L.check(fn(_ptr(x), Cc, _ptr(k), N, S, Cc, _stream()), name)


def instnorm_act_fwd(x, stats, gamma, beta, eps, act, slope):
    _chk_dev(x, gamma, beta, f64=(stats,))
    N, S, Cc = _nsc(x)
    y = new_act(*x.shape, like=x)
    mr = torch.empty((N, Cc, 2), dtype=torch.float32, device=x.device)
    fn, name = _fn("rehr_instnorm_act_fwd", x)
    L.check(fn(_ptr(x), Cc, _ptr(stats), _ptr(gamma), _ptr(beta), _ptr(y), Cc, _ptr(mr), N, S, Cc, eps, act, slope,
               _stream()), name)
    return y, mr


def instnorm_act_bwd(dy, x, mr, gamma, beta, act, slope, want_conv_bias=False):
    """-> (dx, dgamma, dbeta[, dconv_bias]).  want_conv_bias (bf16 only): the column sums of dx -- the gradient of the
    bias of the convolution in front -- formed inside the apply pass instead of by a separate pass over dx."""
    _chk_dev(dy, x, mr, gamma, beta)
    _same_dtype(dy, x)
    N, S, Cc = _nsc(x)
    dx = new_act(*x.shape, like=x)
    dg = torch.empty((Cc,), dtype=torch.float32, device=x.device)
    db = torch.empty((Cc,), dtype=torch.float32, device=x.device)
    red = zeros_f64((N, Cc, 2), x.device)
    if want_conv_bias:
        if x.dtype != torch.bfloat16:
            raise L.RehrsegHipError("the fused conv-bias gradient exists for the bf16 path (fp32: the weight-gradient kernels carry it)")
        dsum = torch.empty((Cc,), dtype=torch.float64, device=x.device)
        dcb = torch.empty((Cc,), dtype=torch.float32, device=x.device)
        L.check(L.load().rehr_instnorm_act_bwd_dbias_bf16(_ptr(dy), Cc, _ptr(x), Cc, _ptr(mr), _ptr(gamma), _ptr(beta),
                                                          _ptr(dx), Cc, _ptr(dg), _ptr(db), _ptr(red), N, S, Cc, act,
                                                          slope, _ptr(dsum), _ptr(dcb), _stream()),
                "rehr_instnorm_act_bwd_dbias_bf16")
        return dx, dg, db, dcb
    fn, name = _fn("rehr_instnorm_act_bwd", x)
    L.check(fn(_ptr(dy), Cc, _ptr(x), Cc, _ptr(mr), _ptr(gamma), _ptr(beta), _ptr(dx), Cc, _ptr(dg), _ptr(db), _ptr(red),
               N, S, Cc, act, slope, _stream()), name)
    return dx, dg, db


def upsample_depth_fwd(x, Do):
    _chk_dev(x)
    N, Cc, Di, H, W = x.shape
    y = new_act(N, Cc, Do, H, W, like=x)
    L.check(L.load().rehr_upsample_depth_fwd_f32(_ptr(x), _ptr(y), N, Di, Do, H * W, Cc, _stream()),
            "rehr_upsample_depth_fwd_f32")
    return y


def upsample_depth_bwd(dy, Di):
    _chk_dev(dy)
    N, Cc, Do, H, W = dy.shape
    dx = new_act(N, Cc, Di, H, W, like=dy)
    L.check(L.load().rehr_upsample_depth_bwd_f32(_ptr(dy), _ptr(dx), N, Di, Do, H * W, Cc, _stream()),
            "rehr_upsample_depth_bwd_f32")
    return dx


def upmix_depth_fwd(g, bias, Do, Cc, KD, pd, act, slope):
    """g (N, KD*Cc, Di, H, W) NDHWC -> y (N, Cc, Do, H, W): depth interpolation + depth-tap sum + bias + act."""
    _chk_dev(g, bias)
    N, _, Di, H, W = g.shape
    y = new_act(N, Cc, Do, H, W, like=g)
    fn, name = _fn("rehr_upmix_depth_fwd", g)
    L.check(fn(_ptr(g), _ptr(bias), _ptr(y), N, Di, Do, H * W, Cc, KD, pd, act, slope, _stream()), name)
    return y


def upmix_depth_bwd(dy, y, Di, KD, pd, act, slope):
    """dg of upmix_depth_fwd from the output gradient dy and the saved output y (dz = dy * act'(y) on the fly)."""
    _chk_dev(dy, y)
    _same_dtype(dy, y)
    N, Cc, Do, H, W = dy.shape
    dg = new_act(N, KD * Cc, Di, H, W, like=dy)
    fn, name = _fn("rehr_upmix_depth_bwd", dy)
    L.check(fn(_ptr(dy), _ptr(y), _ptr(dg), N, Di, Do, H * W, Cc, KD, pd, act, slope, _stream()), name)
    return dg


def channel_sum_actgrad(dy, y, act, slope):
    _chk_dev(dy, y)
    _same_dtype(dy, y)
    N, S, Cc = _nsc(dy)
    out = torch.empty((Cc,), dtype=torch.float32, device=dy.device)
    scratch = torch.empty((Cc,), dtype=torch.float64, device=dy.device)
    fn, name = _fn("rehr_channel_sum_actgrad", dy)
    L.check(fn(_ptr(dy), _ptr(y), Cc, N * S, Cc, act, slope, _ptr(out), _ptr(scratch), _stream()), name)
    return out


def window_stem_assemble(g, mean, bias, B, nwin, act, slope, out_dtype=None):
    """g = three (B*(nwin+3)+1, C, 1, h, w) NDHWC fp32 per-tap responses -> y (B*nwin, C, 4, h, w) (see the header);
    out_dtype bf16: stored for a mixed-precision first block."""
    _chk_dev(*g, mean, bias)
    S, Cc, _, h, w = g[0].shape
    if S != B * (nwin + 3) + 1:
        raise ValueError("window_stem_assemble: slice count")
    if any(t.dtype != torch.float32 for t in g):
        raise L.RehrsegHipError("window_stem_assemble: the per-tap responses are float32")
    bf = out_dtype == torch.bfloat16
    y = new_act(B * nwin, Cc, 4, h, w, like=g[0], dtype=torch.bfloat16 if bf else torch.float32)
    fn = L.load().rehr_window_stem_assemble_bf16 if bf else L.load().rehr_window_stem_assemble_f32
    L.check(fn(_ptr(g[0]), _ptr(g[1]), _ptr(g[2]), _ptr(mean), _ptr(bias), _ptr(y), B, nwin, nwin + 3, h * w, Cc, act,
               slope, _stream()), "rehr_window_stem_assemble")
    return y


def cosdist_stats(x1, x2):
    """(N, 64, D, H, W) NDHWC pair -> stats (N, 64, 3) fp64 = (S12, S11, S22) of the channel-normalised tensors."""
    _chk_dev(x1, x2)
    N, Cc, D, H, W = x1.shape
    stats = torch.empty((N, Cc, 3), dtype=torch.float64, device=x1.device)
    L.check(L.load().rehr_cosdist_stats_f32(_ptr(x1), _ptr(x2), _ptr(stats), N, D * H * W, Cc, _stream()),
            "rehr_cosdist_stats_f32")
    return stats


def cosdist_bwd(x1, x2, stats, scale):
    _chk_dev(x1, x2, f64=(stats,))
    N, Cc, D, H, W = x1.shape
    dx = new_act(N, Cc, D, H, W, like=x1)
    L.check(L.load().rehr_cosdist_bwd_f32(_ptr(x1), _ptr(x2), _ptr(stats), _ptr(dx), N, D * H * W, Cc, float(scale),
                                          _stream()), "rehr_cosdist_bwd_f32")
    return dx


def _uasr_args(om, ue, wu, bu, D):
    _chk_dev(om, ue, wu, bu)
    for t in (om, ue, wu, bu):
        if t.dtype != torch.float32:
            raise L.RehrsegHipError("uasr_mix: float32 operands")
    N, C2, one, H, W = om.shape
    K = ue.shape[1] // D
    if one != 1 or ue.shape != (N, K * D, 1, H, W) or C2 != 2 * K * D or wu.numel() != K or bu.numel() != 1:
        raise ValueError(f"uasr_mix: om {tuple(om.shape)} / ue {tuple(ue.shape)} / D {D} / wu {tuple(wu.shape)}")
    if K not in (4, 8, 16, 32):
        raise NotImplementedError(f"uasr_mix: K = {K} candidates per slice (kernels: 4, 8, 16, 32)")
    return N, K, H, W


def uasr_mix_fwd(om, ue, wu, bu, D):
    """om (N, D*2K, 1, H, W), ue (N, D*K, 1, H, W) NDHWC -> out (N, 2, D, H, W), unc (N, 1, D, H, W) (see the header)."""
    N, K, H, W = _uasr_args(om, ue, wu, bu, D)
    out = torch.empty((N, 2, D, H, W), dtype=torch.float32, device=om.device)
    unc = torch.empty((N, 1, D, H, W), dtype=torch.float32, device=om.device)
    L.check(L.load().rehr_uasr_mix_fwd_f32(_ptr(om), _ptr(ue), _ptr(wu), _ptr(bu), _ptr(out), _ptr(unc), N, K, D, H * W,
                                           _stream()), "rehr_uasr_mix_fwd_f32")
    return out, unc


def uasr_mix_bwd(om, ue, wu, bu, gout, gunc, D):
    """Gradients of uasr_mix_fwd: (dom, due, dwu (K,), dbu (1,)); gout / gunc dense NCDHW."""
    N, K, H, W = _uasr_args(om, ue, wu, bu, D)
    _chk_dev(gout, gunc)
    if gout.shape != (N, 2, D, H, W) or gunc.shape != (N, 1, D, H, W) or not (gout.is_contiguous() and gunc.is_contiguous()):
        raise ValueError("uasr_mix_bwd: gout (N,2,D,H,W) / gunc (N,1,D,H,W), contiguous")
    dom = new_act(N, 2 * K * D, 1, H, W, like=om)
    due = new_act(N, K * D, 1, H, W, like=ue)
    lib = L.load()
    blocks = lib.rehr_uasr_mix_blocks(N, D, H * W)
    partial = torch.empty((blocks, K + 1), dtype=torch.float64, device=om.device)
    L.check(lib.rehr_uasr_mix_bwd_f32(_ptr(om), _ptr(ue), _ptr(wu), _ptr(bu), _ptr(gout), _ptr(gunc), _ptr(dom), _ptr(due),
                                      _ptr(partial), N, K, D, H * W, _stream()), "rehr_uasr_mix_bwd_f32")
    tot = partial.sum(0).float()
    return dom, due, tot[:K], tot[K:]


def quad_maxpool_fwd(x):
    """x (N, C, D, H, W) NDHWC, H and W even -> (y (N*D, C, 2, 2) fp32 NHWC-dense, idx int32 same layout)."""
    _chk_dev(x)
    N, Cc, D, H, W = x.shape
    y = torch.empty((N * D, Cc, 2, 2), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    idx = torch.empty((N * D, 2, 2, Cc), dtype=torch.int32, device=x.device)
    L.check(L.load().rehr_quad_maxpool_fwd_f32(_ptr(x), _ptr(y), C.c_void_p(idx.data_ptr()), N * D, H, W, Cc, _stream()),
            "rehr_quad_maxpool_fwd_f32")
    return y, idx


def quad_maxpool_bwd(dy, idx, shape):
    _chk_dev(dy)
    N, Cc, D, H, W = shape
    dy = dy.contiguous(memory_format=torch.channels_last)
    dx = new_act(N, Cc, D, H, W, like=dy)
    L.check(L.load().rehr_quad_maxpool_bwd_f32(_ptr(dy), C.c_void_p(idx.data_ptr()), _ptr(dx), N * D, H, W, Cc, _stream()),
            "rehr_quad_maxpool_bwd_f32")
    return dx


def act_fwd(x, act, slope):
    _chk_dev(x)
    y = torch.empty_like(x)
    L.check(L.load().rehr_act_fwd_f32(_ptr(x), _ptr(y), x.numel(), act, slope, _stream()), "rehr_act_fwd_f32")
    return y


def act_bwd(dy, y, act, slope):
    _chk_dev(dy, y)
    _same_dtype(dy, y)
    dx = torch.empty_like(y)
    fn, name = _fn("rehr_act_bwd", y)
    L.check(fn(_ptr(dy), _ptr(y), _ptr(dx), y.numel(), act, slope, _stream()), name)
    return dx


def channel_sum(x):
    _chk_dev(x)
    N, S, Cc = _nsc(x)
    out = torch.empty((Cc,), dtype=torch.float32, device=x.device)
    scratch = torch.empty((Cc,), dtype=torch.float64, device=x.device)
    fn, name = _fn("rehr_channel_sum", x)
    L.check(fn(_ptr(x), Cc, N * S, Cc, _ptr(out), 0, _ptr(scratch), _stream()), name)
    return out


def seg_loss_fwd(logits, target, unc):
    """logits (N,C,D,H,W) NDHWC, target/unc (N,S) float32 -> stats double[N*C*3 + 1]."""
    _chk_dev(logits, target, unc)
    N, Cc = logits.shape[0], logits.shape[1]
    S = logits.shape[2] * logits.shape[3] * logits.shape[4]
    stats = torch.empty(N * Cc * 3 + 1, dtype=torch.float64, device=logits.device)
    L.check(L.load().rehr_seg_loss_fwd_f32(_ptr(logits), Cc, _ptr(target), _ptr(unc), N, Cc, S, _ptr(stats),
                                           _stream()), "rehr_seg_loss_fwd_f32")
    return stats


def seg_loss_bwd(logits, target, unc, stats, w_ce, w_dice, smooth, do_bg, grad_out):
    _chk_dev(logits, target, unc, grad_out, f64=(stats,))
    N, Cc, D, H, W = logits.shape
    dl = new_act(N, Cc, D, H, W, like=logits)
    L.check(L.load().rehr_seg_loss_bwd_f32(_ptr(logits), Cc, _ptr(target), _ptr(unc), N, Cc, D * H * W, _ptr(stats),
                                           float(w_ce), float(w_dice), float(smooth), int(do_bg), _ptr(grad_out),
                                           _ptr(dl), Cc, _stream()), "rehr_seg_loss_bwd_f32")
    return dl


SEG_TOPK_MAX_ELEMENTS, SEG_TOPK_MAX_SAMPLES = 1 << 30, 4
SEG_TOPK_STATS = 4      # n_gt, n_eq, the sum above the threshold, the threshold: behind seg_loss_fwd's N*C*3 + 1


def _ndhwc_ld(x, what):
    """The voxel pitch of a logical (N,C,D,H,W) float32 device tensor whose memory is NDHWC: C for a dense one, more
    for a channel slice of a wider NDHWC tensor."""
    if x.dim() != 5 or x.dtype != torch.float32 or not x.is_cuda:
        raise L.RehrsegHipError(f"{what}: float32 (N,C,D,H,W) device tensor (no CPU fallback)")
    N, Cc, D, H, W = x.shape
    ld = x.stride(4) if W > 1 else (x.stride(3) if H > 1 else (x.stride(2) if D > 1 else (x.stride(0) if N > 1 else Cc)))
    want = (D * H * W * ld, 1, H * W * ld, W * ld, ld)
    if ld < Cc or any(n > 1 and s != w for n, s, w in zip(x.shape, x.stride(), want)):
        raise L.RehrsegHipError(f"{what}: NDHWC memory (ops.to_cl) or a channel slice of it, got strides {x.stride()}")
    return ld


def _seg_topk_operands(logits, target, unc, K):
    ld = _ndhwc_ld(logits, "seg_topk")
    N, Cc, D, H, W = logits.shape
    S = D * H * W
    for t, what in ((target, "target"), (unc, "uncertainty")):
        if t is not None:
            _chk_eval(t, torch.float32, f"seg_topk {what}", 2)
            if tuple(t.shape) != (N, S):
                raise L.RehrsegHipError(f"seg_topk: {what} is (N, S) = ({N}, {S}), got {tuple(t.shape)}")
    M = (N * N if unc is not None else N) * S
    if not 2 <= Cc <= 4 or N > SEG_TOPK_MAX_SAMPLES or M > SEG_TOPK_MAX_ELEMENTS:
        raise L.RehrsegHipError("seg_topk: 2..4 classes, at most 4 samples and 2**30 loss-map elements (REHR_ENOSUP)")
    if not 1 <= int(K) <= M:
        raise L.RehrsegHipError(f"seg_topk: K = {K} outside [1, {M}]")
    return ld, N, Cc, S


def seg_topk_workspace(N, Cc, S, with_unc, device):
    """The workspace of seg_topk_fwd / seg_topk_bwd: the loss map, the threshold and the select's own workspace."""
    return _workspace(L.load().rehr_seg_topk_workspace_bytes, (N, Cc, S, int(bool(with_unc))), device,
                      "rehr_seg_topk_workspace_bytes")


def seg_topk_fwd(logits, target, unc, K, workspace=None):
    """logits (N,C,D,H,W) NDHWC or a channel slice of it, target / unc (N,S) float32, K a Python int -> (stats double
    [N*C*3 + 1 + 4], workspace): seg_loss_fwd's statistics, then n_gt, n_eq, the sum of the map above the threshold
    and the threshold (rehr_seg_topk_fwd_f32).  The workspace holds the loss map for seg_topk_bwd.  No host sync."""
    ld, N, Cc, S = _seg_topk_operands(logits, target, unc, K)
    if workspace is None:
        workspace = seg_topk_workspace(N, Cc, S, unc is not None, logits.device)
    _chk_eval(workspace, torch.uint8, "seg_topk workspace", 1)
    stats = torch.empty(N * Cc * 3 + 1 + SEG_TOPK_STATS, dtype=torch.float64, device=logits.device)
    L.check(L.load().rehr_seg_topk_fwd_f32(_ptr(logits), ld, _ptr(target), _ptr(unc), N, Cc, S, int(K), _ptr(stats),
                                           _ptr(workspace), workspace.numel(), _stream()), "rehr_seg_topk_fwd_f32")
    return stats, workspace


def seg_topk_map(workspace, N, S, with_unc):
    """The loss map seg_topk_fwd left in its workspace: float32 (N, S), or (N, N, S) with an uncertainty (a view)."""
    shape = (N, N, S) if with_unc else (N, S)
    n = (N * N if with_unc else N) * S
    return workspace[:4 * n].view(torch.float32).view(shape)


def seg_topk_bwd(logits, target, unc, K, stats, workspace, w_ce, w_dice, smooth, do_bg, grad_out):
    """dlogits of the loss seg_topk_fwd's statistics stand for, times grad_out (a one-element device tensor);
    stats and workspace are the forward's (rehr_seg_topk_bwd_f32)."""
    ld, N, Cc, S = _seg_topk_operands(logits, target, unc, K)
    _chk_dev(grad_out, f64=(stats,))
    _chk_eval(workspace, torch.uint8, "seg_topk workspace", 1)
    dl = new_act(N, Cc, logits.shape[2], logits.shape[3], logits.shape[4], like=logits)
    L.check(L.load().rehr_seg_topk_bwd_f32(_ptr(logits), ld, _ptr(target), _ptr(unc), N, Cc, S, int(K), _ptr(stats),
                                           _ptr(workspace), workspace.numel(), float(w_ce), float(w_dice),
                                           float(smooth), int(do_bg), _ptr(grad_out), _ptr(dl), Cc, _stream()),
            "rehr_seg_topk_bwd_f32")
    return dl


def _ds_levels(logits, targets, uncs, weights, dlogits=None):
    """The host descriptors of one deep-supervision launch.  logits[l] (N,C,d,h,w) NDHWC float32, targets[l] / uncs[l]
    (N,S) float32; a level whose weight is 0 is skipped and may hold None."""
    n = len(logits)
    if not 1 <= n <= L.DS_MAX_LEVELS or len(targets) != n or len(weights) != n or (uncs is not None and len(uncs) != n):
        raise L.RehrsegHipError(f"deep supervision: 1..{L.DS_MAX_LEVELS} levels with one target and one weight each")
    live = [l for l in range(n) if float(weights[l]) != 0.0]
    if not live:
        raise L.RehrsegHipError("deep supervision: every level has weight 0")
    N, Cc = logits[live[0]].shape[:2]
    arr = (L.SegDsLevel * n)()
    for l in live:
        x, t = logits[l], targets[l]
        u = None if uncs is None else uncs[l]
        _chk_dev(x, t, u)
        if x.dtype != torch.float32 or x.dim() != 5 or tuple(x.shape[:2]) != (N, Cc) or \
                not x.permute(0, 2, 3, 4, 1).is_contiguous():
            raise L.RehrsegHipError("deep supervision: float32 NDHWC logits with one (N, C) over all levels")
        d, h, w = x.shape[2:]
        S = d * h * w
        for name, v in (("target", t), ("uncertainty", u)):
            if v is not None and (v.dtype != torch.float32 or tuple(v.shape) != (N, S) or not v.is_contiguous()):
                raise L.RehrsegHipError(f"deep supervision: {name} of level {l} must be contiguous float32 ({N}, {S})")
        arr[l].logits, arr[l].target = x.data_ptr(), t.data_ptr()
        arr[l].unc = None if u is None else u.data_ptr()
        arr[l].S, arr[l].d, arr[l].h, arr[l].w = S, d, h, w
        arr[l].ld = arr[l].ldd = Cc
        arr[l].weight = float(weights[l])
        if dlogits is not None:
            arr[l].dlogits = dlogits[l].data_ptr()
    return arr, n, N, Cc


def seg_loss_ds_fwd(logits, targets, uncs, weights):
    """Every level of a deep-supervision loss in one launch (rehr_seg_loss_ds_fwd_f32) -> stats double
    [levels][N*C*3 + 1], one row per level laid out as seg_loss_fwd's (rows of skipped levels are zero)."""
    arr, n, N, Cc = _ds_levels(logits, targets, uncs, weights)
    dev = next(x for x in logits if x is not None).device
    stats = torch.empty((n, N * Cc * 3 + 1), dtype=torch.float64, device=dev)
    L.check(L.load().rehr_seg_loss_ds_fwd_f32(arr, n, N, Cc, _ptr(stats), _stream()), "rehr_seg_loss_ds_fwd_f32")
    return stats


def seg_loss_ds_bwd(logits, targets, uncs, weights, stats, w_ce, w_dice, smooth, do_bg, grad_out):
    """-> per level grad_out * weight * d(loss_l)/d(logits_l) in one launch; None for a skipped level."""
    _chk_dev(grad_out, f64=(stats,))
    dl = [None if float(w) == 0.0 else new_act(*x.shape, like=x) for x, w in zip(logits, weights)]
    arr, n, N, Cc = _ds_levels(logits, targets, uncs, weights, dl)
    if tuple(stats.shape) != (n, N * Cc * 3 + 1) or not stats.is_contiguous():
        raise L.RehrsegHipError("deep supervision: stats of another launch")
    L.check(L.load().rehr_seg_loss_ds_bwd_f32(arr, n, N, Cc, _ptr(stats), float(w_ce), float(w_dice), float(smooth),
                                              int(do_bg), _ptr(grad_out), _stream()), "rehr_seg_loss_ds_bwd_f32")
    return dl


def label_pyramid(src, extents, tables):
    """Every level of an order-0 label pyramid in one launch (rehr_label_pyramid_f32).  src: contiguous float32 device
    tensor (..., z, y, x); extents[l] = (d, h, w); tables[l] = (iz, iy, ix) device int32 source indices of the three
    axes, whose values the caller has checked against (z, y, x).  -> [(..., d, h, w) float32 per level]."""
    _chk_dev(src)
    if src.dtype != torch.float32 or not src.is_contiguous() or src.dim() < 3:
        raise L.RehrsegHipError("label_pyramid: contiguous float32 (..., z, y, x) source")
    n = len(extents)
    if not 1 <= n <= L.DS_MAX_LEVELS or len(tables) != n:
        raise L.RehrsegHipError(f"label_pyramid: 1..{L.DS_MAX_LEVELS} levels with three index tables each")
    lead = tuple(src.shape[:-3])
    z, y, x = src.shape[-3:]
    B = src.numel() // (z * y * x)
    arr = (L.PyramidLevel * n)()
    outs = []
    for l, (ext, tab) in enumerate(zip(extents, tables)):
        ext = tuple(int(v) for v in ext)
        if len(ext) != 3 or min(ext) < 1 or len(tab) != 3:
            raise L.RehrsegHipError(f"label_pyramid: level {l} needs a positive (d, h, w) and three tables")
        for t, k in zip(tab, ext):
            if t.dtype != torch.int32 or t.device != src.device or tuple(t.shape) != (k,) or not t.is_contiguous():
                raise L.RehrsegHipError(f"label_pyramid: level {l} index tables are int32 [{ext}] on the source's device")
        out = torch.empty(lead + ext, dtype=torch.float32, device=src.device)
        outs.append(out)
        arr[l].dst = out.data_ptr()
        arr[l].d, arr[l].h, arr[l].w = ext
        arr[l].iz, arr[l].iy, arr[l].ix = (t.data_ptr() for t in tab)
    if B == 0:
        return outs
    L.check(L.load().rehr_label_pyramid_f32(_ptr(src), B, z, y, x, arr, n, _stream()), "rehr_label_pyramid_f32")
    return outs


def bce_dice_fwd(x, t):
    """x, t dense (N, C, S) float32 -> stats (C, 4) double = {sum bce, sum p t, sum p^2, sum t^2}."""
    _chk_dev(x, t)
    N, Cc, S = x.shape
    stats = torch.empty((Cc, 4), dtype=torch.float64, device=x.device)
    L.check(L.load().rehr_bce_dice_fwd_f32(_ptr(x), _ptr(t), N, Cc, S, _ptr(stats), _stream()), "rehr_bce_dice_fwd_f32")
    return stats


def bce_dice_bwd(x, t, stats, alpha, beta, grad_out):
    _chk_dev(x, t, grad_out, f64=(stats,))
    N, Cc, S = x.shape
    dx = torch.empty_like(x)
    L.check(L.load().rehr_bce_dice_bwd_f32(_ptr(x), _ptr(t), N, Cc, S, _ptr(stats), float(alpha), float(beta), _ptr(grad_out),
                                           _ptr(dx), _stream()), "rehr_bce_dice_bwd_f32")
    return dx


# ----------------------------------------------------------------------------- training-patch feed (section 8 f-4)
def patch_gather(items, dims, scale=1.0, bias=0.0):
    """One launch cuts len(items) patches out of device-resident volumes (rehr_patch_gather).

    items: (src, base, stride[4], lo[4], hi[4]) per patch; src is a contiguous float32 / uint8 device tensor, base and
    stride count source elements.  Returns float32 [len(items), *dims].  Every address the valid box [lo, hi) can
    produce is checked here against the volume (the kernel trusts its descriptors)."""
    dims = tuple(int(v) for v in dims)
    if len(dims) != 4 or not items:
        raise L.RehrsegHipError("patch_gather: four output axes and at least one item")
    dt = items[0][0].dtype
    if dt not in (torch.float32, torch.uint8):
        raise L.RehrsegHipError(f"patch_gather: float32 or uint8 volumes, got {dt}")
    arr = (L.PatchItem * len(items))()
    for i, (src, base, stride, lo, hi) in enumerate(items):
        if not src.is_cuda or not src.is_contiguous() or src.dtype != dt:
            raise L.RehrsegHipError("patch_gather: contiguous device volumes of one dtype (no CPU fallback)")
        lo_off = hi_off = int(base)
        empty = False
        for k in range(4):
            if not (0 <= lo[k] <= hi[k] <= dims[k]):
                raise L.RehrsegHipError(f"patch_gather: valid box {lo}..{hi} outside the patch {dims}")
            if lo[k] == hi[k]:
                empty = True
                continue
            a, b = int(stride[k]) * int(lo[k]), int(stride[k]) * (int(hi[k]) - 1)
            lo_off += min(a, b)
            hi_off += max(a, b)
        if not empty and (lo_off < 0 or hi_off >= src.numel()):
            raise L.RehrsegHipError(f"patch_gather: item {i} addresses [{lo_off}, {hi_off}] of a {src.numel()}-element volume")
        arr[i].src = src.data_ptr()
        arr[i].base = int(base)
        for k in range(4):
            arr[i].stride[k] = int(stride[k])
            arr[i].lo[k] = int(lo[k])
            arr[i].hi[k] = int(hi[k])
    out = torch.empty((len(items),) + dims, device=items[0][0].device, dtype=torch.float32)
    d = L.PatchGatherDesc()
    d.n_items = len(items)
    for k in range(4):
        d.dims[k] = dims[k]
    d.src_dtype = L.PATCH_U8 if dt == torch.uint8 else L.PATCH_F32
    d.scale, d.bias = float(scale), float(bias)
    d.dst = out.data_ptr()
    d.dst_item_stride = out[0].numel()
    L.check(L.load().rehr_patch_gather(C.byref(d), arr, _stream()), "rehr_patch_gather")
    return out


def axis_resample(x, axis, idx, w, validated=False):
    """y[..., j, ...] = sum_t w[j, t] * x[..., idx[j, t], ...] along `axis` (idx < 0 drops the term); x contiguous float32
    on the device, idx int32 [n_out, taps], w float32 [n_out, taps] (device).  `validated`: the caller has already
    checked idx < x.shape[axis] on the host (saves the device round trip of the check here)."""
    _chk_dev(x, w)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise L.RehrsegHipError("axis_resample: contiguous float32 input")
    if idx.dtype != torch.int32 or idx.shape != w.shape or idx.dim() != 2 or not idx.is_cuda:
        raise L.RehrsegHipError("axis_resample: idx int32 / w float32 tables of one [n_out, taps] shape on the device")
    axis = axis % x.dim()
    n_in = x.shape[axis]
    if not validated and idx.numel() and int(idx.max()) >= n_in:
        raise L.RehrsegHipError("axis_resample: tap index beyond the axis")
    outer = 1
    for s in x.shape[:axis]:
        outer *= s
    inner = 1
    for s in x.shape[axis + 1:]:
        inner *= s
    n_out, taps = idx.shape
    y = torch.empty(x.shape[:axis] + (n_out,) + x.shape[axis + 1:], device=x.device, dtype=torch.float32)
    if y.numel() == 0:
        return y
    L.check(L.load().rehr_axis_resample_f32(_ptr(x), _ptr(y), _ptr(idx.contiguous()), _ptr(w.contiguous()), outer, n_in,
                                            n_out, inner, taps, _stream()), "rehr_axis_resample_f32")
    return y


# ----------------------------------------------------------------------------- training augmentation (augment.hip)
AUG_WARP_SPLINE3, AUG_WARP_LABEL, AUG_WARP_PARAMS = 0, 1, 8
AUG_NOISE, AUG_SCALE, AUG_CONTRAST, AUG_CLIP, AUG_GAMMA, AUG_RETAIN = range(6)
AUG_PW_PARAMS, AUG_STAT_PARTS = 4, 256


def aug_warp2d(src, params, out_hw, mode):
    """src (B, C, Hi, Wi) -> (B, C, Ho, Wo): the in-plane affine of every slice c of item b with params[b] (float64
    [B, AUG_WARP_PARAMS] on the device) -- rehr_aug_warp2d_f32."""
    _chk_eval(src, torch.float32, "aug_warp2d src")
    _chk_eval(params, torch.float64, "aug_warp2d params")
    B, Cc, Hi, Wi = src.shape
    Ho, Wo = (int(v) for v in out_hw)
    if params.shape != (B, AUG_WARP_PARAMS):
        raise L.RehrsegHipError("aug_warp2d: one parameter record per item")
    dst = torch.empty((B, Cc, Ho, Wo), device=src.device, dtype=torch.float32)
    L.check(L.load().rehr_aug_warp2d_f32(_ptr(src), _ptr(dst), _ptr(params), B, Cc, Hi, Wi, Ho, Wo, int(mode),
                                         _stream()), "rehr_aug_warp2d_f32")
    return dst


def aug_stats(x, out=None):
    """x (B, ...) -> float64 (B, 4) {sum, sum of squares, min, max} per item (rehr_aug_stats_f32)."""
    _chk_eval(x, torch.float32, "aug_stats input")
    if out is not None:
        _chk_eval(out, torch.float64, "aug_stats out")
    B = x.shape[0]
    S = x.numel() // B
    work = torch.empty(B * AUG_STAT_PARTS * 4, device=x.device, dtype=torch.float64)
    st = torch.empty((B, 4), device=x.device, dtype=torch.float64) if out is None else out
    L.check(L.load().rehr_aug_stats_f32(_ptr(x), B, S, _ptr(work), _ptr(st), _stream()), "rehr_aug_stats_f32")
    return st


def aug_pointwise(x, op, params, stats0=None, stats1=None):
    """One intensity step in place over x (B, ...) with params float64 [B, AUG_PW_PARAMS] (rehr_aug_pointwise_f32)."""
    _chk_eval(x, torch.float32, "aug_pointwise input")
    for t in (params, stats0, stats1):
        if t is not None:
            _chk_eval(t, torch.float64, "aug_pointwise parameters / statistics")
    B = x.shape[0]
    if params.shape != (B, AUG_PW_PARAMS):
        raise L.RehrsegHipError("aug_pointwise: one parameter record per item")
    L.check(L.load().rehr_aug_pointwise_f32(_ptr(x), B, x.numel() // B, int(op), _ptr(params), _ptr(stats0),
                                            _ptr(stats1), _stream()), "rehr_aug_pointwise_f32")
    return x


# ----------------------------------------------------------------------------- stage-2 validation (seg_eval.hip)
def tta_gather(vol, pad, start, tile, out=None):
    """vol (D, H, W) fp32, constant-padded by `pad` voxels below -> the (8, 1, d, h, w) TTA batch of the tile at
    `start` (padded coordinates): identity, then the mirrorings in itertools.combinations order (rehr_tta_gather_f32)."""
    _chk_eval(vol, torch.float32, "tta_gather volume", 3)
    d, h, w = (int(v) for v in tile)
    if out is None:
        out = torch.empty((8, 1, d, h, w), device=vol.device, dtype=torch.float32)
    elif tuple(out.shape) != (8, 1, d, h, w):
        raise L.RehrsegHipError("tta_gather: out must be (8, 1) + tile")
    _chk_eval(out, torch.float32, "tta_gather out")
    L.check(L.load().rehr_tta_gather_f32(_ptr(vol), _ptr(out), *vol.shape, *(int(v) for v in pad),
                                         *(int(v) for v in start), d, h, w, _stream()), "rehr_tta_gather_f32")
    return out


def tta_blend(pred, logits, counts, start, gaussian=None):
    """Un-mirror the network's (8, C, d, h, w) fp32 output (any strides), average, weight and add it into the fp16
    accumulators logits [C, D, H, W] / counts [D, H, W] at `start` (rehr_tta_blend_f16acc)."""
    if not pred.is_cuda or pred.dtype != torch.float32 or pred.dim() != 5 or pred.shape[0] != 8:
        raise L.RehrsegHipError("tta_blend: the prediction is an (8, C, d, h, w) float32 device tensor")
    _chk_eval(logits, torch.float16, "tta_blend logits", 4)
    _chk_eval(counts, torch.float16, "tta_blend counts", 3)
    C_, d, h, w = pred.shape[1:]
    if logits.shape[0] != C_ or tuple(logits.shape[1:]) != tuple(counts.shape):
        raise L.RehrsegHipError("tta_blend: logits [C, D, H, W] and counts [D, H, W] of the prediction's C")
    if gaussian is not None:
        _chk_eval(gaussian, torch.float16, "tta_blend gaussian", 3)
        if tuple(gaussian.shape) != (d, h, w):
            raise L.RehrsegHipError("tta_blend: the Gaussian has the tile's shape")
    strides = (C.c_int64 * 5)(*pred.stride())
    L.check(L.load().rehr_tta_blend_f16acc(_ptr(pred), strides, C_, d, h, w, _ptr(gaussian), _ptr(logits),
                                           _ptr(counts), *counts.shape, *(int(v) for v in start), _stream()),
            "rehr_tta_blend_f16acc")


def seg_eval_finalize(logits, counts, stats, crop=None, labels=None, gt=None):
    """logits [2, D, H, W] /= counts in place; stats (int64 [4], zeroed): [0] set on an inf, [1..3] += the Dice terms
    sum(p * gt), sum(p), sum(gt) against gt; labels (uint8, the crop's shape) = the argmax inside `crop`, a tuple of
    slices of (D, H, W) (None: the whole volume) (rehr_seg_eval_finalize_f16)."""
    _chk_eval(logits, torch.float16, "seg_eval_finalize logits", 4)
    _chk_eval(counts, torch.float16, "seg_eval_finalize counts", 3)
    _chk_eval(stats, torch.int64, "seg_eval_finalize stats", 1)
    if logits.shape[0] != 2:
        raise L.RehrsegHipError("seg_eval_finalize: 2 classes")
    if tuple(logits.shape[1:]) != tuple(counts.shape) or stats.numel() < 4:
        raise L.RehrsegHipError("seg_eval_finalize: counts [D, H, W] of the logits, 4 stats")
    dims = tuple(counts.shape)
    crop = crop or tuple(slice(None) for _ in dims)
    lo, size = [], []
    for sl, n in zip(crop, dims):
        a, b, _ = sl.indices(n)
        lo.append(a)
        size.append(b - a)
    for t, what in ((labels, "labels"), (gt, "gt")):
        if t is not None:
            _chk_eval(t, torch.uint8, f"seg_eval_finalize {what}", 3)
            if tuple(t.shape) != tuple(size):
                raise L.RehrsegHipError(f"seg_eval_finalize: {what} has the crop's shape {tuple(size)}")
    L.check(L.load().rehr_seg_eval_finalize_f16(_ptr(logits), _ptr(counts), *dims, *lo, *size, _ptr(labels), _ptr(gt),
                                                _ptr(stats), _stream()), "rehr_seg_eval_finalize_f16")


# ----------------------------------------------------------------------------- boundary metrics (seg_surface.hip)
SEG_SURFACE_MAX_AXIS = 2048     # REHR_SEG_SURFACE_MAX_AXIS
SEG_SURFACE_MAX_VOXELS = 1 << 30


def seg_surface_check_extent(shape):
    """Raises for a (D, H, W) the surface kernels do not take; no launch, no allocation."""
    dims = tuple(int(v) for v in shape)
    if len(dims) != 3 or min(dims) < 1:
        raise L.RehrsegHipError(f"surface metrics: a (D, H, W) volume with every axis >= 1, got {dims}")
    if max(dims) > SEG_SURFACE_MAX_AXIS or dims[0] * dims[1] * dims[2] > SEG_SURFACE_MAX_VOXELS:
        raise L.RehrsegHipError(f"surface metrics: unsupported extent {dims}: every axis <= {SEG_SURFACE_MAX_AXIS} and "
                                f"at most 2**30 voxels (REHR_ENOSUP)")
    return dims


def _surface_workspace(dims, device):
    return _workspace(L.load().rehr_seg_surface_workspace_bytes, dims, device, "rehr_seg_surface_workspace_bytes")


def seg_surface_distances(pred, gt, spacing, counts, workspace=None):
    """pred, gt: uint8 (D, H, W), non-zero = foreground; spacing (sd, sh, sw) as fp32 values.  Returns (dist fp32
    [2, D*H*W], workspace): dist[0] the distance of every surface voxel of pred to gt's surface, dist[1] the reverse,
    +inf at the other voxels; counts (int64 [2], zeroed) += the two surface sizes (rehr_seg_surface_dist_f32)."""
    _chk_eval(pred, torch.uint8, "seg_surface_distances pred", 3)
    _chk_eval(gt, torch.uint8, "seg_surface_distances gt", 3)
    _chk_eval(counts, torch.int64, "seg_surface_distances counts", 1)
    dims = seg_surface_check_extent(pred.shape)
    if tuple(gt.shape) != dims or counts.numel() != 2:
        raise L.RehrsegHipError("seg_surface_distances: gt has pred's shape, 2 counts")
    if workspace is None:
        workspace = _surface_workspace(dims, pred.device)
    dist = torch.empty((2, dims[0] * dims[1] * dims[2]), device=pred.device, dtype=torch.float32)
    L.check(L.load().rehr_seg_surface_dist_f32(_ptr(pred), _ptr(gt), *dims, *(float(s) for s in spacing), _ptr(dist),
                                               _ptr(counts), _ptr(workspace), workspace.numel(), _stream()),
            "rehr_seg_surface_dist_f32")
    return dist, workspace


def seg_surface_reduce(dist, dist_sorted, counts, out, workspace):
    """out (int64 [3], the bits of three fp64) = hd, hd95, assd from dist [2, N], its ascending sort [2 * N] and the
    counts, all on the device (rehr_seg_surface_reduce_f64)."""
    _chk_eval(dist, torch.float32, "seg_surface_reduce dist", 2)
    _chk_eval(dist_sorted, torch.float32, "seg_surface_reduce sorted", 1)
    _chk_eval(counts, torch.int64, "seg_surface_reduce counts", 1)
    _chk_eval(out, torch.int64, "seg_surface_reduce out", 1)
    if dist.shape[0] != 2 or dist_sorted.numel() != dist.numel() or counts.numel() != 2 or out.numel() != 3:
        raise L.RehrsegHipError("seg_surface_reduce: dist [2, N], sorted [2 * N], 2 counts, 3 outputs")
    L.check(L.load().rehr_seg_surface_reduce_f64(_ptr(dist), _ptr(dist_sorted), _ptr(counts), dist.shape[1], _ptr(out),
                                                 _ptr(workspace), workspace.numel(), _stream()),
            "rehr_seg_surface_reduce_f64")


# ----------------------------------------------------------------------------- connected components (seg_components.hip)
SEG_CC_MAX_VOXELS = 1 << 30
SEG_CC_CONNECTIVITIES = (6, 18, 26)


def seg_cc_check_extent(shape):
    """Raises for a (D, H, W) the component kernels do not take; no launch, no allocation."""
    dims = tuple(int(v) for v in shape)
    if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] > SEG_CC_MAX_VOXELS:
        raise L.RehrsegHipError(f"connected components: unsupported extent {dims}: a (D, H, W) volume with every "
                                f"axis >= 1 and at most 2**30 voxels (REHR_ENOSUP)")
    return dims


def _cc_connectivity(connectivity):
    if connectivity not in SEG_CC_CONNECTIVITIES:
        raise L.RehrsegHipError(f"connected components: connectivity 6, 18 or 26, got {connectivity!r}")
    return int(connectivity)


def seg_cc_workspace(dims, device):
    """The workspace of seg_cc_roots / seg_cc_lesion for a (D, H, W) volume."""
    return _workspace(L.load().rehr_seg_cc_workspace_bytes, dims, device, "rehr_seg_cc_workspace_bytes")


def seg_cc_roots(mask, connectivity, workspace=None):
    """mask: uint8 (D, H, W), non-zero = foreground.  Returns (roots int32 (D, H, W), workspace): the smallest linear
    index of every voxel's component, -1 at background (rehr_seg_cc_roots_i32)."""
    _chk_eval(mask, torch.uint8, "seg_cc_roots mask", 3)
    dims = seg_cc_check_extent(mask.shape)
    conn = _cc_connectivity(connectivity)
    if workspace is None:
        workspace = seg_cc_workspace(dims, mask.device)
    roots = torch.empty(dims, device=mask.device, dtype=torch.int32)
    L.check(L.load().rehr_seg_cc_roots_i32(_ptr(mask), *dims, conn, _ptr(roots), _ptr(workspace), workspace.numel(),
                                           _stream()), "rehr_seg_cc_roots_i32")
    return roots, workspace


def seg_cc_compact(roots, count):
    """roots: seg_cc_roots' map.  Returns labels int32 of its shape, 1..n in the order of the roots and 0 at
    background; count (int64 [1], zeroed) += n.  The prefix sum between is torch's cumsum (rehr_seg_cc_compact_i32)."""
    _chk_eval(roots, torch.int32, "seg_cc_compact roots", 3)
    _chk_eval(count, torch.int64, "seg_cc_compact count", 1)
    seg_cc_check_extent(roots.shape)
    if count.numel() != 1:
        raise L.RehrsegHipError("seg_cc_compact: 1 count")
    n = roots.numel()
    flat = roots.view(-1)
    rank = torch.cumsum((flat == torch.arange(n, device=roots.device, dtype=torch.int32)).to(torch.int32), 0,
                        dtype=torch.int32)
    labels = torch.empty_like(roots)
    L.check(L.load().rehr_seg_cc_compact_i32(_ptr(roots), n, _ptr(rank), _ptr(labels), _ptr(count), _stream()),
            "rehr_seg_cc_compact_i32")
    return labels


def seg_cc_lesion(roots_pred, roots_gt, out, workspace=None):
    """out (int64 [8], zeroed) += n_pred, n_gt, tp_pred, tp_gt, the sizes of the largest component of either map, the
    foreground of gt inside pred's largest, the foreground of gt (rehr_seg_cc_lesion_i64).  Returns the two packed
    keys (size << 32) | (0xffffffff - root) of the largest components as an int64 [2] view of the workspace."""
    _chk_eval(roots_pred, torch.int32, "seg_cc_lesion roots_pred", 3)
    _chk_eval(roots_gt, torch.int32, "seg_cc_lesion roots_gt", 3)
    _chk_eval(out, torch.int64, "seg_cc_lesion out", 1)
    dims = seg_cc_check_extent(roots_pred.shape)
    if tuple(roots_gt.shape) != dims or out.numel() != 8:
        raise L.RehrsegHipError("seg_cc_lesion: roots_gt has roots_pred's shape, 8 outputs")
    if workspace is None:
        workspace = seg_cc_workspace(dims, roots_pred.device)
    L.check(L.load().rehr_seg_cc_lesion_i64(_ptr(roots_pred), _ptr(roots_gt), roots_pred.numel(), _ptr(out),
                                            _ptr(workspace), workspace.numel(), _stream()), "rehr_seg_cc_lesion_i64")
    return workspace[:16].view(torch.int64)


# ----------------------------------------------------------------------------- intensity normalisation (intensity_norm.hip)
ORDER_STATS_MAX_RANKS, PERCENTILE_MAX_Q = 8, 4
INTENSITY_MAX_VOXELS, INTENSITY_MAX_ITEMS = 1 << 30, 65535
INTENSITY_PERCENTILE, INTENSITY_ZEROONE = 0, 1


def _item_runs(x, what):
    """(B, S, stride) of a float32 device tensor whose items x[b] are dense runs of S elements, stride elements apart
    (a contiguous (B, ...) tensor, or channel 0 of a contiguous (B, C, ...) one)."""
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() < 1:
        raise L.RehrsegHipError(f"{what}: float32 device tensor (B, ...) (no CPU fallback)")
    B = x.shape[0]
    S = x.numel() // max(B, 1)
    if B < 1 or S < 1 or not x[0].is_contiguous():
        raise L.RehrsegHipError(f"{what}: at least one item, every item a dense run")
    if B > INTENSITY_MAX_ITEMS or S > INTENSITY_MAX_VOXELS:
        raise L.RehrsegHipError(f"{what}: at most 65535 items of at most 2**30 elements (REHR_ENOSUP)")
    return B, S, (x.stride(0) if B > 1 else S)


def order_stats_workspace(B, R, device):
    """The workspace of order_stats for B items and R ranks."""
    return _workspace(L.load().rehr_order_stats_workspace_bytes, (B, R), device, "rehr_order_stats_workspace_bytes")


def order_stats(x, ranks, out=None, workspace=None):
    """x (B, ...) float32 on the device, every item a dense run (see _item_runs); ranks: up to 8 Python ints in
    [0, S).  Returns float32 (B, R): out[b][r] = sort(x[b])[ranks[r]], NaN for an item with a NaN
    (rehr_order_stats_f32).  No host sync."""
    B, S, stride = _item_runs(x, "order_stats")
    ranks = [int(k) for k in ranks]
    R = len(ranks)
    if not 1 <= R <= ORDER_STATS_MAX_RANKS or min(ranks) < 0 or max(ranks) >= S:
        raise L.RehrsegHipError(f"order_stats: 1..8 ranks inside [0, {S}), got {ranks}")
    if out is None:
        out = torch.empty((B, R), device=x.device, dtype=torch.float32)
    _chk_eval(out, torch.float32, "order_stats out", 2)
    if tuple(out.shape) != (B, R):
        raise L.RehrsegHipError("order_stats: out is (B, R)")
    if workspace is None:
        workspace = order_stats_workspace(B, R, x.device)
    L.check(L.load().rehr_order_stats_f32(_ptr(x), B, S, stride, (C.c_int64 * R)(*ranks), R, _ptr(out),
                                          _ptr(workspace), workspace.numel(), _stream()), "rehr_order_stats_f32")
    return out


def percentile_plan(S, q):
    """numpy.percentile's virtual indices for S elements, in Python floats: (ranks [k0, k1 per q], t per q) with
    h = q / 100 * (S - 1), k0 = floor(h), k1 = min(k0 + 1, S - 1), t = h - k0."""
    ranks, ts = [], []
    for p in q:
        p = float(p)
        if not 0.0 <= p <= 100.0:
            raise ValueError(f"percentiles must be in the range [0, 100], got {p!r}")
        h = (p / 100.0) * (S - 1)
        k0 = min(int(h // 1), S - 1)
        ranks += [k0, min(k0 + 1, S - 1)]
        ts.append(h - k0)
    return ranks, ts


def percentile_bounds(stats, t, strictly_positive=False, out=None):
    """stats: order_stats' (B, 2 Q) for percentile_plan's ranks, t: its Q fractions.  Returns float64 (B, Q): numpy's
    'linear' percentiles; with strictly_positive a negative first column becomes 0 (rehr_percentile_f64)."""
    _chk_eval(stats, torch.float32, "percentile_bounds stats", 2)
    t = [float(v) for v in t]
    B, Q = stats.shape[0], len(t)
    if not 1 <= Q <= PERCENTILE_MAX_Q or stats.shape[1] != 2 * Q:
        raise L.RehrsegHipError("percentile_bounds: 1..4 percentiles, two order statistics each")
    if out is None:
        out = torch.empty((B, Q), device=stats.device, dtype=torch.float64)
    _chk_eval(out, torch.float64, "percentile_bounds out", 2)
    if tuple(out.shape) != (B, Q):
        raise L.RehrsegHipError("percentile_bounds: out is (B, Q)")
    L.check(L.load().rehr_percentile_f64(_ptr(stats), B, Q, (C.c_double * Q)(*t), int(bool(strictly_positive)),
                                         _ptr(out), _stream()), "rehr_percentile_f64")
    return out


def intensity_apply(x, bounds, mode, out=None):
    """y[b] = (clip(x[b], lo, hi) - lo) / (hi - lo) (INTENSITY_PERCENTILE) or (x[b] - lo) / (hi - lo)
    (INTENSITY_ZEROONE) with {lo, hi} = the first two entries of bounds[b] (float64 (B, >= 2) on the device, rows
    dense) rounded to fp32.  x as order_stats'; out: a contiguous tensor of B * S elements, or x itself for in place
    (rehr_intensity_apply_f32).  Returns out."""
    B, S, stride = _item_runs(x, "intensity_apply")
    if not bounds.is_cuda or bounds.dtype != torch.float64 or bounds.dim() != 2 or bounds.shape[0] != B or \
            bounds.shape[1] < 2 or bounds.stride(1) != 1 or (B > 1 and bounds.stride(0) < 2):
        raise L.RehrsegHipError("intensity_apply: bounds float64 (B, >= 2) on the device")
    if out is None:
        out = torch.empty((B, S), device=x.device, dtype=torch.float32)
    if out is x:
        ystride = stride
    else:
        _chk_eval(out, torch.float32, "intensity_apply out")
        if out.numel() != B * S:
            raise L.RehrsegHipError("intensity_apply: out holds B * S elements")
        ystride = S
    L.check(L.load().rehr_intensity_apply_f32(_ptr(x), _ptr(out), B, S, stride, ystride, int(mode), _ptr(bounds),
                                              bounds.stride(0) if B > 1 else 2, _stream()),
            "rehr_intensity_apply_f32")
    return out


# ----------------------------------------------------------------------------- class locations (class_locations.hip)
CLASS_LOCATIONS_MAX_VOXELS, CLASS_LOCATIONS_MAX_RANKS = (1 << 31) - 1, 1 << 20


def class_locations_workspace(N, device):
    """The workspace of class_locations for a label run of N voxels."""
    return _workspace(L.load().rehr_class_locations_workspace_bytes, (N,), device,
                      "rehr_class_locations_workspace_bytes")


def class_locations(label, value, u, count=None, index=None, workspace=None):
    """label: a contiguous uint8 device tensor of any shape (16-byte aligned, not written); value: 0..255, or -1 for
    any non-zero label; u: R 32-bit fractions as a contiguous int32 device tensor that carries the bits of numpy's
    uint32 (torch has no arithmetic on uint32, and nothing here needs any: `torch.from_numpy(a.view(np.int32))`).
    Returns (count int64 [1], index int32 [R]) on the device: count = the voxels that match, index[j] = the linear
    index of the ((u[j] * count) >> 32)-th of them in ascending order, -1 everywhere when there is none
    (rehr_class_locations_u8).  count / index: where to write them, e.g. slices of one buffer.  No host sync."""
    _chk_eval(label, torch.uint8, "class_locations label")
    _chk_eval(u, torch.int32, "class_locations u", 1)
    N, R, value = label.numel(), u.numel(), int(value)
    if not 1 <= N <= CLASS_LOCATIONS_MAX_VOXELS or not 1 <= R <= CLASS_LOCATIONS_MAX_RANKS or not -1 <= value <= 255:
        raise L.RehrsegHipError(f"class_locations: 1..2**31 - 1 voxels, 1..2**20 fractions, a value in [-1, 255]; got "
                                f"{N}, {R}, {value}")
    if count is None:
        count = torch.empty(1, dtype=torch.int64, device=label.device)
    if index is None:
        index = torch.empty(R, dtype=torch.int32, device=label.device)
    _chk_eval(count, torch.int64, "class_locations count", 1)
    _chk_eval(index, torch.int32, "class_locations index", 1)
    if count.numel() != 1 or index.numel() != R:
        raise L.RehrsegHipError("class_locations: 1 count, one index per fraction")
    if workspace is None:
        workspace = class_locations_workspace(N, label.device)
    L.check(L.load().rehr_class_locations_u8(_ptr(label), N, value, _ptr(u), R, _ptr(count), _ptr(index),
                                             _ptr(workspace), workspace.numel(), _stream()), "rehr_class_locations_u8")
    return count, index


# ----------------------------------------------------------------------------- stage-1 -> stage-2 handoff (sr_volume.hip)
def minmax_new(device, pairs=1):
    """`pairs` empty {min, max} code pairs (int32 storage of the kernels' order-preserving uint32 codes)."""
    mm = torch.empty(2 * pairs, device=device, dtype=torch.int32)
    mm[0::2].fill_(-1)   # 0xffffffff: above every code
    mm[1::2].zero_()
    return mm


def minmax_decode(mm):
    """The float32 values behind a buffer of min / max codes (device arithmetic, no host read)."""
    return torch.where(mm < 0, mm & 0x7FFFFFFF, ~mm).view(torch.float32)


def _chk_mm(mm, what):
    if not mm.is_cuda or mm.dtype != torch.int32 or mm.numel() != 2 or not mm.is_contiguous():
        raise L.RehrsegHipError(f"{what}: a {{min, max}} code pair (2 x int32 on the device)")


def minmax(x, out=None):
    """Fold min / max of the float32 device tensor x into the code pair `out` (a fresh one by default)
    (rehr_minmax_f32)."""
    _chk_eval(x, torch.float32, "minmax input")
    if out is None:
        out = minmax_new(x.device)
    _chk_mm(out, "minmax out")
    L.check(L.load().rehr_minmax_f32(_ptr(x), x.numel(), _ptr(out), _stream()), "rehr_minmax_f32")
    return out


def sr_window_gather(vol, w0, b):
    """vol (X, Y, Z, C) fp32 -> the network input of the windows [w0, w0 + b) of apply_to_vol_flavr: logical
    (b, C, 4, Xp, Yp), NDHWC memory, in-plane zero-padded to multiples of 16 (rehr_sr_window_gather_f32)."""
    _chk_eval(vol, torch.float32, "sr_window_gather volume", 4)
    X, Y, Z, Cc = vol.shape
    w0, b = int(w0), int(b)
    if Cc not in (1, 2) or Z < 2 or w0 < 0 or b < 1 or w0 + b > Z - 1:
        raise L.RehrsegHipError(f"sr_window_gather: windows [{w0}, {w0 + b}) of a {tuple(vol.shape)} volume")
    Xp, Yp = X + (-X) % 16, Y + (-Y) % 16
    out = torch.empty((b, 4, Xp, Yp, Cc), device=vol.device, dtype=torch.float32)
    L.check(L.load().rehr_sr_window_gather_f32(_ptr(vol), _ptr(out), X, Y, Z, Cc, w0, b, Xp, Yp, _stream()),
            "rehr_sr_window_gather_f32")
    return out.permute(0, 4, 1, 2, 3)


def sr_volume_scatter(net, in_minmax, w0, img, seg, out_minmax):
    """The network output net (b, C, n_out, >= X, >= Y) fp32 (any strides) of the windows from w0 on -> its slices of
    img (Zo, Y, X) fp32 after inv_normalize with the input's min / max codes, seg (uint8, or None) = channel 1 > 0, and
    the min / max of what was written folded into out_minmax (rehr_sr_volume_scatter_f32)."""
    if not net.is_cuda or net.dtype != torch.float32 or net.dim() != 5:
        raise L.RehrsegHipError("sr_volume_scatter: the network output is a 5-D float32 device tensor")
    _chk_eval(img, torch.float32, "sr_volume_scatter img", 3)
    _chk_mm(in_minmax, "sr_volume_scatter in_minmax")
    _chk_mm(out_minmax, "sr_volume_scatter out_minmax")
    b, Cc, n_out = net.shape[:3]
    Zo, Y, X = img.shape
    if Zo % n_out or net.shape[3] < X or net.shape[4] < Y or w0 < 0 or (int(w0) + b) * n_out > Zo:
        raise L.RehrsegHipError(f"sr_volume_scatter: output {tuple(net.shape)} at window {w0} into {tuple(img.shape)}")
    if seg is not None:
        _chk_eval(seg, torch.uint8, "sr_volume_scatter seg", 3)
        if tuple(seg.shape) != tuple(img.shape) or Cc < 2:
            raise L.RehrsegHipError("sr_volume_scatter: seg has img's shape and needs a second channel")
    strides = (C.c_int64 * 5)(*net.stride())
    L.check(L.load().rehr_sr_volume_scatter_f32(_ptr(net), strides, b, Cc, n_out, X, Y, int(w0), Zo // n_out,
                                                _ptr(in_minmax), _ptr(img), _ptr(seg), _ptr(out_minmax), _stream()),
            "rehr_sr_volume_scatter_f32")


def stage2_prep(img, minmax_codes, taps):
    """zeroonenorm (min / max from the code pair) and the blur `taps` (float32 device vector, L <= 32) along the first
    axis of img (X, ...) fp32, in one pass (rehr_stage2_prep_f32)."""
    _chk_eval(img, torch.float32, "stage2_prep img")
    _chk_eval(taps, torch.float32, "stage2_prep taps", 1)
    _chk_mm(minmax_codes, "stage2_prep minmax")
    if img.dim() < 2 or img.numel() == 0:
        raise L.RehrsegHipError("stage2_prep: a non-empty image of at least two axes")
    out = torch.empty_like(img)
    X = img.shape[0]
    L.check(L.load().rehr_stage2_prep_f32(_ptr(img), _ptr(minmax_codes), _ptr(taps), taps.numel(), _ptr(out), X,
                                          img.numel() // X, _stream()), "rehr_stage2_prep_f32")
    return out


def stage2_unc_u8(u, minmax_codes):
    """(zeroonenorm(u) * 255).astype('uint8') of the float32 device tensor u (rehr_stage2_unc_u8_f32)."""
    _chk_eval(u, torch.float32, "stage2_unc_u8 input")
    _chk_mm(minmax_codes, "stage2_unc_u8 minmax")
    out = torch.empty(u.shape, device=u.device, dtype=torch.uint8)
    L.check(L.load().rehr_stage2_unc_u8_f32(_ptr(u), _ptr(minmax_codes), _ptr(out), u.numel(), _stream()),
            "rehr_stage2_unc_u8_f32")
    return out


# ----------------------------------------------------------------------------- stage-1 volume preparation (stage1_volume.hip)
def zoom_depth(vol, idx, w, nn):
    """scipy.ndimage.zoom along the slice axis of vol (X, Y, n, C) fp32, C in {1, 2}, from the tables of
    utils.sr_utils.zoom_taps on the device: idx int32 [Z, 4], w float64 [Z, 4], nn int32 [Z].  Returns img (X, Y, Z)
    fp32 (order 3 of channel 0) and label (X, Y, Z) uint8 (order 0 of channel 1; None with C == 1)
    (rehr_zoom_depth_f32)."""
    _chk_eval(vol, torch.float32, "zoom_depth volume", 4)
    _chk_eval(idx, torch.int32, "zoom_depth idx", 2)
    _chk_eval(w, torch.float64, "zoom_depth w", 2)
    _chk_eval(nn, torch.int32, "zoom_depth nn", 1)
    X, Y, n, Cc = vol.shape
    Z = idx.shape[0]
    if Cc not in (1, 2) or X * Y * n == 0 or Z < 1 or tuple(idx.shape) != (Z, 4) or tuple(w.shape) != (Z, 4) or \
            nn.numel() != Z:
        raise L.RehrsegHipError(f"zoom_depth: a non-empty (x, y, n, 1 or 2) volume and tables [Z, 4], [Z, 4], [Z], got "
                                f"{tuple(vol.shape)}, {tuple(idx.shape)}, {tuple(w.shape)}, {tuple(nn.shape)}")
    img = torch.empty((X, Y, Z), device=vol.device, dtype=torch.float32)
    label = torch.empty((X, Y, Z), device=vol.device, dtype=torch.uint8) if Cc == 2 else None
    L.check(L.load().rehr_zoom_depth_f32(_ptr(vol), X * Y, n, Cc, _ptr(idx), _ptr(w), _ptr(nn if Cc == 2 else None), Z,
                                         _ptr(img), _ptr(label), _stream()), "rehr_zoom_depth_f32")
    return img, label


def bspline_prefilter(x, axis):
    """The cubic B-spline coefficients of the float32 device tensor x along `axis` (mirror boundaries, fp64 recursion,
    one rounding to fp32): scipy.ndimage.spline_filter1d(x, 3, axis, mode='mirror')
    (rehr_bspline_prefilter_axis_f64acc_f32)."""
    _chk_eval(x, torch.float32, "bspline_prefilter input")
    if x.dim() < 1 or x.numel() == 0:
        raise L.RehrsegHipError("bspline_prefilter: a non-empty tensor")
    axis = axis % x.dim()
    outer = 1
    for s in x.shape[:axis]:
        outer *= s
    inner = 1
    for s in x.shape[axis + 1:]:
        inner *= s
    y = torch.empty_like(x)
    L.check(L.load().rehr_bspline_prefilter_axis_f64acc_f32(_ptr(x), _ptr(y), outer, x.shape[axis], inner, _stream()),
            "rehr_bspline_prefilter_axis_f64acc_f32")
    return y


def blur_to_slices(img, taps, axis):
    """The blur `taps` (float32 device vector, L <= 32, zero-padded 'same' cross-correlation) of img (X, Y, Z) fp32 along
    x (axis 0; returns (Z, X, Y)) or y (axis 1; returns (Z, Y, X)) (rehr_blur_to_slices_f32)."""
    _chk_eval(img, torch.float32, "blur_to_slices img", 3)
    _chk_eval(taps, torch.float32, "blur_to_slices taps", 1)
    if axis not in (0, 1) or img.numel() == 0 or taps.numel() == 0:
        raise L.RehrsegHipError("blur_to_slices: axis 0 (x) or 1 (y) of a non-empty (x, y, z) image")
    X, Y, Z = img.shape
    out = torch.empty((Z, X, Y) if axis == 0 else (Z, Y, X), device=img.device, dtype=torch.float32)
    L.check(L.load().rehr_blur_to_slices_f32(_ptr(img), _ptr(taps), taps.numel(), _ptr(out), X, Y, Z, axis, _stream()),
            "rehr_blur_to_slices_f32")
    return out


# ----------------------------------------------------------------------------- stage-1 validation (sr_metrics.hip)
def sr_metrics(pred, target, seg_logits=None, seg_target=None, data_range=1.0):
    """Per-sample quality sums of the (N, D, H, W) views pred (fp32 or bf16) against target (fp32), and of the foreground
    seg_logits > 0 (pred's dtype) against seg_target > 0.5 (fp32): an (N, 7) float64 device tensor {sum |p - t|,
    sum (p - t)^2, sum of the SSIM index over the valid 11x11 windows of every slice, their number, intersection,
    predicted and target foreground counts}.  The views are read through their strides, nothing is copied and nothing
    is read back (rehr_sr_metrics_f32 / _bf16)."""
    if (seg_logits is None) != (seg_target is None):
        raise L.RehrsegHipError("sr_metrics: seg_logits and seg_target come together")
    for t, what in ((pred, "pred"), (target, "target"), (seg_logits, "seg_logits"), (seg_target, "seg_target")):
        if t is None:
            continue
        if not torch.is_tensor(t) or not t.is_cuda:
            raise L.RehrsegHipError(f"sr_metrics {what}: a device tensor (no CPU fallback)")
        if t.dim() != 4 or tuple(t.shape) != tuple(pred.shape):
            raise L.RehrsegHipError(f"sr_metrics {what}: an (N, D, H, W) view of the prediction's shape "
                                    f"{tuple(pred.shape)}, got {tuple(t.shape)}")
        if t.device != pred.device:
            raise L.RehrsegHipError("sr_metrics: operands on one device")
    if pred.dtype not in (torch.float32, torch.bfloat16):
        raise L.RehrsegHipError(f"sr_metrics pred: float32 or bfloat16, got {pred.dtype}")
    if target.dtype != torch.float32 or (seg_target is not None and seg_target.dtype != torch.float32):
        raise L.RehrsegHipError("sr_metrics: the targets are float32")
    if seg_logits is not None and seg_logits.dtype != pred.dtype:
        raise L.RehrsegHipError("sr_metrics seg_logits: the prediction's dtype")
    N, D, H, W = (int(v) for v in pred.shape)
    lib = L.load()
    ws = _workspace(lib.rehr_sr_metrics_workspace_bytes, (N, D, H, W), pred.device, "rehr_sr_metrics_workspace_bytes")
    stats = torch.empty((N, 7), dtype=torch.float64, device=pred.device)
    strides = lambda t: (C.c_int64 * 4)(*t.stride()) if t is not None else None  # noqa: E731
    fn, name = _fn("rehr_sr_metrics", pred)
    L.check(fn(_ptr(pred), strides(pred), _ptr(target), strides(target), _ptr(seg_logits), strides(seg_logits),
               _ptr(seg_target), strides(seg_target), N, D, H, W, float(data_range), _ptr(stats), _ptr(ws), ws.numel(),
               _stream()), name)
    return stats


# ----------------------------------------------------------------------------- stage-1 structure losses (sr_losses.hip)
def _structure_loss_operands(what, input, target, weights):
    """-> (the two operands as 5-D views, the logical shape, the four weights as floats)."""
    for t, name in ((input, "input"), (target, "target")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise L.RehrsegHipError(f"{what} {name}: a device tensor (no CPU fallback)")
        if t.dtype != torch.float32:
            raise L.RehrsegHipError(f"{what} {name}: float32, got {t.dtype}")
    if input.dim() not in (4, 5) or tuple(input.shape) != tuple(target.shape):
        raise L.RehrsegHipError(f"{what}: input and target of one shape (N, C, D, H, W) or (N, C, H, W), got "
                                f"{tuple(input.shape)} and {tuple(target.shape)}")
    if input.device != target.device:
        raise L.RehrsegHipError(f"{what}: operands on one device")
    if input.dim() == 4:
        input, target = input.unsqueeze(2), target.unsqueeze(2)
    weights = tuple(float(w) for w in weights)
    if len(weights) != 4:
        raise L.RehrsegHipError(f"{what}: four weights (l1, l2, ssim, sobel)")
    return input, target, tuple(int(v) for v in input.shape), weights


def _strides5(t):
    return (C.c_int64 * 5)(*t.stride())


def structure_loss_fwd(input, target, weights, data_range=1.0, need_grad=True):
    """loss = l1 mean|p - t| + l2 mean (p - t)^2 + ssim (1 - mean SSIM) + sobel mean|G(p) - G(t)| of the fp32 device
    views input / target, (N, C, D, H, W) or (N, C, H, W), read through their strides (rehr_structure_loss_fwd_f32).
    weights = (l1, l2, ssim, sobel).  -> (loss: 0-dim float32, stats: (N, 4) float64 per-sample sums, fields: what
    structure_loss_bwd needs of the SSIM term, or None), all on the device; nothing is read back."""
    x, t, shape, w = _structure_loss_operands("structure_loss_fwd", input, target, weights)
    lib = L.load()
    ws = _workspace(lib.rehr_structure_loss_workspace_bytes, shape, x.device, "rehr_structure_loss_workspace_bytes")
    stats = torch.empty((shape[0], 4), dtype=torch.float64, device=x.device)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    fields = (torch.empty(shape[:3] + (3,) + shape[3:], dtype=torch.float32, device=x.device)
              if (need_grad and w[2] != 0.0) else None)
    L.check(lib.rehr_structure_loss_fwd_f32(_ptr(x), _strides5(x), _ptr(t), _strides5(t), *shape, *w, float(data_range),
                                            _ptr(stats), _ptr(loss), _ptr(fields), _ptr(ws), ws.numel(), _stream()),
            "rehr_structure_loss_fwd_f32")
    return loss, stats, fields


def structure_loss_bwd(input, target, weights, fields, grad_out, out=None):
    """grad_out (one fp32 device element) * d loss / d input of structure_loss_fwd's loss, contiguous in input's shape
    (or written into `out` through its strides); fields: structure_loss_fwd's for the same operands and weights."""
    x, t, shape, w = _structure_loss_operands("structure_loss_bwd", input, target, weights)
    for g, name in ((grad_out, "grad_out"), (fields, "fields"), (out, "out")):
        if g is None:
            continue
        if not torch.is_tensor(g) or not g.is_cuda or g.dtype != torch.float32:
            raise L.RehrsegHipError(f"structure_loss_bwd {name}: a float32 device tensor")
    if grad_out is None or grad_out.numel() != 1:
        raise L.RehrsegHipError("structure_loss_bwd grad_out: one element")
    if w[2] != 0.0 and (fields is None or tuple(fields.shape) != shape[:3] + (3,) + shape[3:] or not fields.is_contiguous()):
        raise L.RehrsegHipError("structure_loss_bwd fields: structure_loss_fwd's (N, C, D, 3, H, W) tensor")
    if out is None:
        out = torch.empty(tuple(input.shape), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != tuple(input.shape):
        raise L.RehrsegHipError("structure_loss_bwd out: input's shape")
    o = out.unsqueeze(2) if out.dim() == 4 else out
    L.check(L.load().rehr_structure_loss_bwd_f32(_ptr(x), _strides5(x), _ptr(t), _strides5(t), *shape, *w,
                                                 _ptr(fields if w[2] != 0.0 else None), _ptr(grad_out), _ptr(o),
                                                 _strides5(o), _stream()), "rehr_structure_loss_bwd_f32")
    return out


# ----------------------------------------------------------------------------- sr_head.2 on the bf16 matrix cores
def _thin5_ws(d, dev, f32=False):
    fn = L.load().rehr_conv5_thin_f32_workspace_bytes if f32 else L.load().rehr_conv5_thin_workspace_bytes
    n = int(fn(C.byref(d)))
    if n < 0:
        L.check(n, "rehr_conv5_thin_workspace_bytes")
    return torch.empty((n + 3) // 4, dtype=torch.float32, device=dev), n


USE_THIN5_F32 = True   # sr_head.2 of the fp32 path on the fp32 matrix cores (False: the VALU kernels of direct_conv.hip)


@functools.lru_cache(maxsize=None)
def _thin5_library_takes(x_shape, w_shape, pad, dtype):
    if dtype not in (torch.bfloat16, torch.float32) or len(w_shape) != 5 or w_shape[1] != x_shape[1]:
        return False
    lib = L.load()
    fn = lib.rehr_conv5_thin_supported if dtype == torch.bfloat16 else lib.rehr_conv5_thin_f32_supported
    return bool(fn(C.byref(_shape_desc(x_shape, w_shape, (1, 1, 1), pad))))


def thin5_supported(x_shape, w_shape, pad, dtype=torch.bfloat16):
    """The shapes the matrix-core kernels of thin_conv_{bf16,f32}.hip take, as the library says (remembered per shape:
    fused_conv3d asks at every call of a thin layer)."""
    if dtype == torch.float32 and not USE_THIN5_F32:
        return False
    return _thin5_library_takes(tuple(x_shape), tuple(w_shape), tuple(pad), dtype)


def thin5_fwd(x, w, bias):
    """y (fp32) = conv3d(x (bf16 or fp32 NDHWC), w, bias) for sr_head.2 (rehr_conv5_thin_fwd_{bf16,f32})."""
    _chk_dev(x, w, bias)
    N, Cin, D, H, W = x.shape
    y = new_act(N, 2, D, H, W, like=x, dtype=torch.float32)
    d = _direct_desc(x, w.contiguous(), bias, y, (1, 1, 1), (2, 2, 2), 0, 0.0, None, 0)
    f32 = x.dtype == torch.float32
    ws, n = _thin5_ws(d, x.device, f32)
    fn, name = _fn("rehr_conv5_thin_fwd", x)
    L.check(fn(C.byref(d), _ptr(ws), n, _stream()), name)
    return y


def thin5_dgrad(dy, w, dtype=torch.bfloat16):
    """dx (NDHWC, 16 channels, `dtype`) of sr_head.2 from dY (fp32 NDHWC, 2 channels)."""
    _chk_dev(dy, w)
    if dy.dtype != torch.float32:
        raise L.RehrsegHipError("thin5_dgrad: fp32 output gradient")
    N, _, D, H, W = dy.shape
    dx = new_act(N, 16, D, H, W, like=dy, dtype=dtype)
    d = _direct_desc(dx, w.contiguous(), None, dy, (1, 1, 1), (2, 2, 2), 0, 0.0, None, 0)
    ws, n = _thin5_ws(d, dy.device, dtype == torch.float32)
    fn, name = _fn("rehr_conv5_thin_dgrad", dx)
    L.check(fn(C.byref(d), _ptr(dx), 16, _ptr(ws), n, _stream()), name)
    return dx


def thin5_wgrad(x, w, dy, want_bias=False):
    """(dw (2,16,5,5,5), db) fp32 of sr_head.2 from x (bf16 or fp32) and dY (fp32)."""
    _chk_dev(x, w, dy)
    if dy.dtype != torch.float32:
        raise L.RehrsegHipError("thin5_wgrad: fp32 output gradient")
    d = _direct_desc(x, w.contiguous(), None, dy, (1, 1, 1), (2, 2, 2), 0, 0.0, None, 0)
    ws, n = _thin5_ws(d, x.device, x.dtype == torch.float32)
    dw = torch.empty_like(w, memory_format=torch.contiguous_format)
    db = torch.empty(2, dtype=torch.float32, device=x.device) if want_bias else None
    fn, name = _fn("rehr_conv5_thin_wgrad", x)
    L.check(fn(C.byref(d), _ptr(dw), _ptr(db), _ptr(ws), n, _stream()), name)
    return dw, db
