"""A red-zone allocator for the code under test.

``Guard(device)`` is a TorchDispatchMode.  While it is active, every tensor the test or the package allocates on ``device``
through one of the intercepted ops lives inside a larger base buffer:

    [ 64 KiB red zone | payload, rounded up to 64 KiB | 64 KiB red zone ]

The whole base buffer is filled with one fixed bit pattern per dtype before the payload is handed out: a NaN with a
recognisable payload for floating types, the byte 0x5A for integer, byte and bool types.  ``data_ptr()`` of a guarded tensor
is 64 KiB past the (256-byte aligned) start of its base buffer, so the 16-byte alignment the kernels assume holds.

Intercepted:
  * ``empty`` / ``new_empty`` / ``empty_like`` / ``empty_strided`` (contiguous results): the payload KEEPS the pattern, so an
    output element no kernel wrote, or a scratch row that is consumed but never produced, reaches the result as NaN;
  * every copy that lands on the device -- ``_to_copy`` (the tests' ``.to(dev)``, and dtype conversions on the device such as
    ``.bfloat16()``), ``clone`` (``.contiguous()``) -- and the factories ``zeros`` / ``ones`` / ``full`` (+ ``_like`` /
    ``new_`` forms), ``randn`` / ``rand`` / ``randint``: the op runs as usual and its (contiguous) result is moved into a
    guarded buffer, so the values are the op's own and the red zones hold the pattern.

What the guard can see:
  * a WRITE outside a buffer changes a red zone: ``check()`` compares every red zone bit for bit with the pattern (integer
    compare, never ``isnan``: a NaN with another payload is a write) and reports shape, dtype, side and the first offset hit;
  * a READ outside a buffer, or of a never-written ``empty`` element, is visible only when it reaches a result: there it is a
    NaN (or a wild integer) against the reference comparison the test already makes.  A kernel that relies on
    ``0 * garbage`` therefore fails, as the project's "mask the bits" rule wants.

What it cannot see: an access that lands more than 64 KiB before, or more than 64 KiB past the rounded-up end of, its buffer;
reads that are masked by a select (those are correct); tensors allocated inside an op the mode does not intercept (the
temporaries of torch's own kernels); allocations made before the mode was entered (``functional.workspace``: poison it with
``poison_workspace``).

Guarded tensors are views into their base buffer (``storage_offset() != 0``, the storage is longer than the tensor), so code
that identifies a tensor by its storage (``functional.cat_of_skip``) does not accept them.
"""
import torch
from torch.utils._python_dispatch import TorchDispatchMode

RED_ZONE = 64 * 1024          # bytes on each side; also the granule the payload is rounded up to

_F32, _F16, _BF16, _F64, _BYTE = 0x7FDEAD42, 0x7EDA, 0x7FDA, 0x7FFDEAD42DEAD421, 0x5A
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def pattern_bits(dtype):
    """the poison of `dtype` as an unsigned integer of the dtype's width, or None for a dtype the guard does not handle"""
    if dtype == torch.float32:
        return _F32
    if dtype == torch.bfloat16:
        return _BF16
    if dtype == torch.float16:
        return _F16
    if dtype == torch.float64:
        return _F64
    if dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.bool):
        return int.from_bytes(bytes([_BYTE]) * dtype.itemsize, "little")
    return None


def _as_ints(t):
    """the bits of `t` (any strides) as integers of the same width"""
    return t.view(_INT_VIEW[t.dtype.itemsize])


def _signed(bits, width):
    return bits - (1 << (8 * width)) if width > 1 and bits >> (8 * width - 1) else bits


def poison_(t):
    """fill `t` (any strides) with the pattern of its dtype, in place"""
    _as_ints(t).fill_(_signed(pattern_bits(t.dtype), t.dtype.itemsize))
    return t


def poisoned(shape, dtype, device):
    """a fresh UNGUARDED tensor that holds the pattern everywhere"""
    return poison_(torch.empty(shape, dtype=dtype, device=device))


def holds_pattern(t):
    """True when every element of `t` (any strides) still holds the pattern of its dtype, bit for bit"""
    return bool((_as_ints(t) == _signed(pattern_bits(t.dtype), t.dtype.itemsize)).all())


def poison_workspace(Fn, dev):
    """fill the process-wide scratch buffer of `functional` with the fp32 pattern: a split-K slab or partial row that is read
    before this call's kernels wrote it is then a NaN, not whatever the last test left there"""
    return poison_(Fn.workspace(dev))


class GuardViolation(AssertionError):
    pass


class _Record:
    __slots__ = ("base", "nbytes", "shape", "dtype", "op")

    def __init__(self, base, nbytes, shape, dtype, op):
        self.base, self.nbytes, self.shape, self.dtype, self.op = base, nbytes, tuple(shape), dtype, op

    def zones(self):
        """(side, integer view of the zone); the trailing zone starts right behind the payload's last element"""
        iv = _INT_VIEW[self.dtype.itemsize]
        return (("before", self.base[:RED_ZONE].view(iv)), ("after", self.base[RED_ZONE + self.nbytes:].view(iv)))

    def name(self):
        return f"{self.op} {list(self.shape)} {str(self.dtype).replace('torch.', '')}"


aten = torch.ops.aten
_EMPTY = {aten.empty.memory_format, aten.new_empty.default, aten.empty_like.default, aten.empty_strided.default}
_REHOME = {aten._to_copy.default, aten.clone.default,
           aten.zeros.default, aten.ones.default, aten.full.default,
           aten.zeros_like.default, aten.ones_like.default, aten.full_like.default,
           aten.new_zeros.default, aten.new_ones.default, aten.new_full.default,
           aten.randn.default, aten.randn.generator, aten.rand.default, aten.rand.generator,
           aten.randint.default, aten.randint.low, aten.randint.generator, aten.randint.low_generator}


def _contiguous_strides(size):
    st, acc = [], 1
    for n in reversed(size):
        st.append(acc)
        acc *= max(int(n), 1)
    return tuple(reversed(st))


class Guard(TorchDispatchMode):
    def __init__(self, device):
        super().__init__()
        self.device = torch.device(device)
        self.records = []

    # ---------------------------------------------------------------------------------------------------- allocation
    def _mine(self, device):
        d = torch.device(device) if device is not None else torch.device("cpu")
        if d.type != self.device.type:
            return False
        return d.index is None or self.device.index is None or d.index == self.device.index

    def alloc(self, size, dtype, op="empty"):
        """a guarded, contiguous tensor of `size` whose payload holds the pattern; None when the guard does not handle it"""
        size = tuple(int(s) for s in size)
        bits = pattern_bits(dtype)
        numel = 1
        for s in size:
            numel *= s
        if bits is None or numel == 0:
            return None
        nbytes = numel * dtype.itemsize
        body = -(-nbytes // RED_ZONE) * RED_ZONE
        raw = torch.empty(2 * RED_ZONE + body + 256, dtype=torch.uint8, device=self.device)
        skip = -raw.data_ptr() % 256          # 0 on the GPU (the caching allocator hands out 512-byte multiples); the CPU aligns to 64
        base = raw[skip:skip + 2 * RED_ZONE + body]
        base.view(_INT_VIEW[dtype.itemsize]).fill_(_signed(bits, dtype.itemsize))
        self.records.append(_Record(base, nbytes, size, dtype, op))
        return base[RED_ZONE:RED_ZONE + nbytes].view(dtype).view(size)

    def _empty(self, func, args, kwargs):
        """(size, dtype) of an intercepted empty-like call whose result is contiguous and on the device, else None"""
        if kwargs.get("layout") not in (None, torch.strided):
            return None
        if func is aten.empty.memory_format:
            size, dtype, device = args[0], kwargs.get("dtype") or torch.get_default_dtype(), kwargs.get("device")
            ok = kwargs.get("memory_format") in (None, torch.contiguous_format)
        elif func is aten.empty_strided.default:
            size, dtype, device = args[0], kwargs.get("dtype") or torch.get_default_dtype(), kwargs.get("device")
            ok = tuple(args[1]) == _contiguous_strides(size)
        elif func is aten.new_empty.default:
            size, dtype, device = args[1], kwargs.get("dtype") or args[0].dtype, kwargs.get("device") or args[0].device
            ok = True
        else:
            src = args[0]
            size, dtype, device = src.shape, kwargs.get("dtype") or src.dtype, kwargs.get("device") or src.device
            mf = kwargs.get("memory_format")
            ok = mf == torch.contiguous_format or (mf in (None, torch.preserve_format) and src.is_contiguous())
        return (size, dtype) if ok and self._mine(device) else None

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func in _EMPTY:
            want = self._empty(func, args, kwargs)
            out = self.alloc(want[0], want[1], func.__name__.split(".")[0]) if want else None
            return out if out is not None else func(*args, **kwargs)
        out = func(*args, **kwargs)
        if func in _REHOME and isinstance(out, torch.Tensor) and self._mine(out.device) and out.layout == torch.strided \
                and out.is_contiguous():
            home = self.alloc(out.shape, out.dtype, func.__name__.split(".")[0])
            if home is not None:
                home.copy_(out)
                return home
        return out

    # --------------------------------------------------------------------------------------------------------- check
    def violations(self):
        """one line per red zone that no longer holds its pattern"""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        flags, where = [], []
        for rec in self.records:
            want = _signed(pattern_bits(rec.dtype), rec.dtype.itemsize)
            for side, zone in rec.zones():
                flags.append((zone != want).any())
                where.append((rec, side, zone, want))
        if not flags:
            return []
        hit = torch.stack(flags).cpu().tolist()
        lines = []
        for bad, (rec, side, zone, want) in zip(hit, where):
            if not bad:
                continue
            idx = (zone != want).nonzero().flatten()
            first, last, n = int(idx[0]), int(idx[-1]), int(idx.numel())
            if side == "before":      # report the element nearest the payload first: that is where an under-run starts
                off = f"{zone.numel() - last} element(s) before the first element (reaches back {zone.numel() - first})"
            else:
                off = f"{first} element(s) past the last element (reaches {last})"
            lines.append(f"{rec.name()}: red zone {side} the buffer was written, {n} element(s), first at {off}, "
                         f"bits 0x{int(zone[last if side == 'before' else first]) & ((1 << 8 * rec.dtype.itemsize) - 1):x}")
        return lines

    def check(self):
        """raise GuardViolation when any red zone of any buffer handed out so far was written"""
        lines = self.violations()
        if lines:
            raise GuardViolation("write outside a guarded buffer:\n  " + "\n  ".join(lines))
        return len(self.records)

    def reset(self):
        self.records.clear()
