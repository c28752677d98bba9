"""Guard bands and poisoned payloads around the allocations a block of test code makes -- a plain helper module (no
conftest, no pytest settings), used from a fixture of the test file that wants it:

    with guarded_alloc.Guarded() as ga:              # Guarded(skew=16): payloads 16 bytes off their 256-byte alignment
        x = ga.guarded(host_tensor)                  # a test input: the same values between two NaN guards
        y, stats = ops.conv_forward(x, ...)          # every torch.empty / empty_like / zeros in there is wrapped
        ga.check()                                   # synchronises; every guard must still hold the fill word

While the context is active torch.empty, torch.empty_like and torch.zeros are replaced for tensors of the wrapped device
types ("cuda" by default; the host test passes devices=("cpu",)).  A wrapped allocation is ONE flat buffer

    [ guard 64 KiB (+ skew) | payload | guard 64 KiB (+ up to 15 bytes to the next 16) ]

and the tensor handed out is an as_strided view of the payload with the shape, strides and dtype the real call would have
given (they are taken from the real call on the "meta" device, so memory_format= and channels_last_3d survive).  64 KiB is
one 128-voxel x 128-channel fp32 tile, the largest unit a single block of the convolution kernels stores.  Guards, and
the payloads of empty / empty_like, hold the 32-bit word FILL = 0x7FC57FC5: a quiet NaN as fp32 and as either bf16 half
(two of them read as 3.0e307 in an fp64, whose exponent is wider: finite, but no sum or square survives it unnoticed),
so an element a kernel leaves unwritten, or reads from outside its tensor, shows in the result; the payload of zeros is
zero.  The payload's data_ptr() stays 16-byte aligned.

hip_backend's pooled fp64 accumulators (zeros_f64) would bypass the wrapper -- they are slices of one chunk that was
zeroed long ago -- so the context sets hip_backend._ZERO_CHUNK to 0 (every accumulator then comes from torch.zeros),
empties hip_backend._zero_pool and forgets the kept weight forms on entry and on exit (no form from outside is used
inside, none from inside survives).  All of it is restored on exit, also when the body raises.

check() compares integers (a NaN is unequal to itself) and names the first allocation whose guard changed by shape and
dtype, the side, and the byte offset from the payload."""
import torch

from rehrseg_amd import hip_backend

GUARD = 64 * 1024
FILL = 0x7FC57FC5
_PATCHED = ("empty", "empty_like", "zeros")


def _round_up(n, m):
    return -(-n // m) * m


class Guarded:
    def __init__(self, skew=0, devices=("cuda",)):
        if skew % 16 or skew < 0:
            raise ValueError("skew keeps the payload 16-byte aligned: a non-negative multiple of 16")
        self.skew, self.devices = skew, tuple(devices)
        self.allocs = []          # (flat uint8 buffer, payload start, payload end, shape, dtype)
        self._patterns = {}
        self._saved = None

    # ------------------------------------------------------------------ context
    def __enter__(self):
        if self._saved is not None:
            raise RuntimeError("Guarded is not re-entrant")
        self._saved = ({n: getattr(torch, n) for n in _PATCHED}, hip_backend._ZERO_CHUNK, hip_backend._zero_pool)
        self._real = self._saved[0]
        hip_backend.invalidate_weight_forms()
        hip_backend._ZERO_CHUNK, hip_backend._zero_pool = 0, {}
        torch.empty = self._wrap("empty", False)
        torch.empty_like = self._wrap("empty_like", False)
        torch.zeros = self._wrap("zeros", True)
        return self

    def __exit__(self, *exc):
        real, chunk, pool = self._saved
        for n, f in real.items():
            setattr(torch, n, f)
        hip_backend._ZERO_CHUNK, hip_backend._zero_pool = chunk, pool
        hip_backend.invalidate_weight_forms()
        self._saved = None
        return False

    # ------------------------------------------------------------------ allocation
    def _wrap(self, name, zero):
        real = self._real[name]

        def alloc(*args, **kw):
            dev = kw.get("device")
            if dev is None and name == "empty_like":
                dev = args[0].device
            if (dev is None or torch.device(dev).type not in self.devices or kw.get("out") is not None or
                    kw.get("pin_memory") or kw.get("layout", torch.strided) is not torch.strided):
                return real(*args, **kw)
            meta = real(*args, **dict(kw, device="meta", requires_grad=False))
            out = self._alloc(tuple(meta.shape), tuple(meta.stride()), meta.dtype, torch.device(dev), zero)
            return out.requires_grad_() if kw.get("requires_grad") else out

        alloc.__name__ = "guarded_" + name
        return alloc

    def _alloc(self, shape, strides, dtype, device, zero):
        if self._saved is None:
            raise RuntimeError("guarded allocations are made inside the context")
        item = self._real["empty"]((), dtype=dtype).element_size()
        extent = 0 if 0 in shape else 1 + sum((n - 1) * s for n, s in zip(shape, strides))
        lo = GUARD + self.skew
        hi = lo + extent * item
        total = _round_up(hi, 16) + GUARD
        words = self._real["empty"](total // 4, dtype=torch.int32, device=device)
        words.fill_(FILL)
        flat = words.view(torch.uint8)
        if zero:
            flat[lo:hi].zero_()
        out = flat[lo:hi].view(dtype).as_strided(shape, strides)
        assert extent == 0 or (out.data_ptr() % 16 == 0 and out.data_ptr() == flat.data_ptr() + lo), "payload alignment"
        self.allocs.append((flat, lo, hi, shape, dtype))
        return out

    def guarded(self, t, device="cuda:0"):
        """Host tensor `t` (dense in its own strides, e.g. channels_last_3d) copied into a guarded allocation on `device`."""
        out = self._alloc(tuple(t.shape), tuple(t.stride()), t.dtype, torch.device(device), False)
        out.copy_(t.detach())
        return out

    # ------------------------------------------------------------------ check
    def _pattern(self, device, n):
        pat = self._patterns.get(device)
        if pat is None or pat.numel() < n:
            pat = self._real["empty"](_round_up(n, 4) // 4 + 8, dtype=torch.int32, device=device).fill_(FILL).view(torch.uint8)
            self._patterns[device] = pat
        return pat

    def check(self):
        """Every guard of every allocation made so far still holds the fill word (compared as integers)."""
        if any(f.is_cuda for f, *_ in self.allocs):
            torch.cuda.synchronize()
        for flat, lo, hi, shape, dtype in self.allocs:
            for side, a, b in (("before", 0, lo), ("after", hi, flat.numel())):
                got = flat[a:b]
                want = self._pattern(flat.device, b - a + 4)[a % 4:a % 4 + (b - a)]
                if torch.equal(got, want):
                    continue
                at = int((got != want).nonzero()[0])
                where = f"{lo - (a + at)} bytes before its start" if side == "before" else f"{at} bytes past its end"
                raise AssertionError(f"guard {side} the {dtype} allocation of shape {shape} changed {where} "
                                     f"(payload {hi - lo} bytes; byte {int(got[at]):#04x}, fill {int(want[at]):#04x})")
        return len(self.allocs)
