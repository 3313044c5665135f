"""Memory-contract helpers for the kernel tests (device-agnostic: the CPU test of this module runs them on CPU tensors).

A kernel's contract has two halves the value tests do not see: which bytes it may WRITE and which bytes its result may
DEPEND on.  Both are checked with tensors that live in the middle of a larger allocation the test owns:

  guarded(...)   an output: the view handed to the kernel sits between a front and a back band, every byte of the arena
                 (the view's own previous contents included) holds a sentinel byte.  assert_untouched() compares the arena
                 AS BYTES with the sentinel everywhere outside the write set the test declares.
  poisoned(...)  an input: the declared read set holds the test data (pad columns up to `ld` zero, as include/tdc_hip.h
                 promises the kernels), everything around it a poison byte.  A test runs the call twice - surroundings
                 ZERO, then NAN_FF - and asserts bit-identical, finite outputs.

NAN_FF (0xFF bytes) is NaN as fp16, bf16, fp32 and e4m3 at once and -1 as int32 (an over-read index array shows too).
No test writes or reads outside an allocation it owns: a stray access lands in a band and is reported, never faults.
"""
import sys

import torch

ZERO = 0x00
NAN_FF = 0xFF
PATTERNS = (ZERO, NAN_FF)


def _round_up(a, b):
    return (a + b - 1) // b * b


class Arena:
    """[front band | rows x ld elements | back band] as one flat uint8 tensor; `view` = the [rows, cols] window."""

    def __init__(self, shape, dtype, device, front_rows, back_rows, ld, fill, align):
        shape = tuple(int(s) for s in shape)
        self.shape = shape
        self.rows = shape[0]
        self.cols = 1
        for s in shape[1:]:
            self.cols *= s
        self.ld = self.cols if ld is None else int(ld)
        assert self.ld >= self.cols and self.rows >= 0
        assert self.ld == self.cols or len(shape) == 2, "a padded leading dimension needs a 2-D shape"
        self.dtype, self.fill = dtype, int(fill)
        self.item = torch.empty((), dtype=dtype).element_size()
        self.ldb = self.ld * self.item
        self.front = _round_up(int(front_rows) * self.ldb, align)
        self.back = _round_up(int(back_rows) * self.ldb, align)
        self.nbytes = self.rows * self.ldb
        self.buf = torch.full((self.front + self.nbytes + self.back,), self.fill, dtype=torch.uint8, device=device)
        body = self.buf[self.front:self.front + self.nbytes].view(dtype).view(self.rows, self.ld)
        self.full = body                                 # [rows, ld]: pad columns included
        self.view = body[:, :self.cols] if self.ld != self.cols else body.view(shape)

    def _byte_mask(self, written):
        """bool [rows, ldb]: True where the declared write set allows a change"""
        dev = self.buf.device
        m = torch.zeros(self.rows, self.ld, dtype=torch.bool, device=dev)
        if written is None:
            m[:, :self.cols] = True
        else:
            w = torch.as_tensor(written, device=dev)
            assert w.dtype == torch.bool, "written_mask must be boolean"
            if w.dim() == 1:
                assert w.numel() == self.rows, "row mask of the wrong length"
                m[:, :self.cols] = w[:, None]
            else:
                w = w.reshape(self.rows, -1)
                assert w.shape[1] in (self.cols, self.ld), "element mask must be [rows, cols] or [rows, ld]"
                m[:, :w.shape[1]] = w
        return m.repeat_interleave(self.item, dim=1)

    def violations(self, written=None, limit=8):
        """positions (row, column) relative to the view, in elements, of sentinel bytes that changed outside `written`"""
        if written is None and self.ld == self.cols:         # the whole view is the write set: only the two bands can be wrong
            lo, hi = self.buf[:self.front], self.buf[self.front + self.nbytes:]
            bad = torch.cat([torch.nonzero(lo != self.fill).reshape(-1),
                             torch.nonzero(hi != self.fill).reshape(-1) + self.front + self.nbytes])
            return self._positions(bad, limit)
        allowed = torch.zeros_like(self.buf, dtype=torch.bool)
        allowed[self.front:self.front + self.nbytes] = self._byte_mask(written).reshape(-1)
        return self._positions(torch.nonzero((self.buf != self.fill) & ~allowed).reshape(-1), limit)

    def _positions(self, bad, limit):
        n = int(bad.numel())
        out = []
        for off in bad[:limit * self.item].tolist():
            rel = off - self.front
            pos = (rel // self.ldb, (rel % self.ldb) // self.item)
            if pos not in out:
                out.append(pos)
        return n, out[:limit]


def guarded(shape, dtype, device, front_rows, back_rows, ld=None, fill=NAN_FF, align=256):
    """-> (view, arena).  view: `shape` (2-D [rows, cols] with row stride `ld` when ld is given), pre-filled with the sentinel
    like the bands and the pad columns cols .. ld around it.  The band heights are counted in rows of `ld` elements (a 1-D
    shape (n,) is n rows of one element) and rounded up so that the view starts on an `align`-byte boundary."""
    a = Arena(shape, dtype, device, front_rows, back_rows, ld, fill, align)
    return a.view, a


def assert_untouched(arena, written_mask=None, what="output"):
    """Every byte of the arena outside the declared write set still holds the sentinel.  written_mask: None = the whole
    logical view [rows, :cols]; a bool [rows] = those rows (columns < cols); a bool [rows, cols] or [rows, ld] = elements."""
    n, pos = arena.violations(written_mask)
    if n:
        raise AssertionError("%s: %d byte(s) written outside the declared write set; first (row, col) relative to the view: %s"
                             % (what, n, ", ".join("(%d, %d)" % p for p in pos)))


def assert_unchanged(arena, before, written_mask=None, what="in/out operand"):
    """For an operand that is read AND written (an in-place update inside a poisoned arena): every byte outside the declared
    write set equals `before` (arena.buf.clone() taken before the call) - bands, pad columns and the rows the call must keep."""
    keep = torch.ones_like(arena.buf, dtype=torch.bool)
    keep[arena.front:arena.front + arena.nbytes] = ~arena._byte_mask(written_mask).reshape(-1)
    bad = torch.nonzero((arena.buf != before) & keep).reshape(-1)
    if bad.numel():
        pos = [((o - arena.front) // arena.ldb, ((o - arena.front) % arena.ldb) // arena.item) for o in bad[:8].tolist()]
        raise AssertionError("%s: %d byte(s) changed outside the declared write set; first (row, col) relative to the view: %s"
                             % (what, int(bad.numel()), ", ".join("(%d, %d)" % p for p in pos)))


def poisoned(data, front_rows, back_rows, ld=None, fill=NAN_FF, rows=None, total_rows=None, pad="zero", align=256):
    """-> (view, arena) for an INPUT: `data` [n, ...] is the declared read set.  Its rows sit at `rows` (default 0 .. n-1) of
    a `total_rows`-row matrix (default n) whose other rows - the gaps of a row map, rows no index names - hold the poison
    byte, like the bands.  Pad columns cols .. ld of the declared rows are zero (pad="zero": the header's promise for
    activation / weight matrices) or poison (pad="poison": columns the kernel is not given)."""
    n = data.shape[0]
    total = n if total_rows is None else int(total_rows)
    a = Arena((total,) + tuple(data.shape[1:]), data.dtype, data.device, front_rows, back_rows, ld, fill, align)
    idx = torch.arange(n, device=data.device) if rows is None else torch.as_tensor(rows, device=data.device).long()
    assert idx.numel() == n and (n == 0 or (int(idx.min()) >= 0 and int(idx.max()) < total))
    if n:
        if pad == "zero" and a.ld != a.cols:
            a.full[idx] = 0
        a.full[idx, :a.cols] = data.reshape(n, a.cols)
    return a.view, a


def same_bits(a, b):
    """bit-for-bit equality (NaN == NaN of the same payload, -0 != +0)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous(), b.contiguous()
    if a.numel() == 0:
        return True
    return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def all_finite(t):
    if t.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.bool):
        return True
    return bool(torch.isfinite(t.float()).all())


class _TorchProxy:
    """`torch` as a tdc_video_amd module sees it, with empty / empty_like replaced"""

    def __init__(self, real, empty, empty_like):
        self.__dict__["_real"] = real
        self.__dict__["empty"] = empty
        self.__dict__["empty_like"] = empty_like

    def __getattr__(self, name):
        return getattr(self._real, name)


def _byte_fill(t, pattern):
    if t.numel():
        assert t.is_contiguous()
        t.reshape(-1).view(torch.uint8).fill_(pattern)
    return t


def poison_empty(monkeypatch, pattern, guard_bytes=0, prefix="tdc_video_amd"):
    """Replace torch.empty / torch.empty_like as seen by the loaded `tdc_video_amd` modules (through pytest's monkeypatch:
    undone when the test ends) with an allocation followed by a byte fill - the state of a recycled allocator block.
    guard_bytes > 0: every such tensor is the view of a guarded arena with bands of that many bytes; the arenas are
    appended to the returned list for assert_untouched (write set: the whole tensor)."""
    real = torch
    arenas = []

    def empty(*size, **kw):
        if "out" in kw:
            return real.empty(*size, **kw)
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        if guard_bytes and len(size) >= 1 and not kw.get("pin_memory", False):
            dtype = kw.get("dtype") or real.get_default_dtype()
            item = real.empty((), dtype=dtype).element_size()
            rows = size[0]
            rowb = item
            for s in size[1:]:
                rowb *= int(s)
            band = (guard_bytes + rowb - 1) // max(rowb, 1)
            a = Arena(size, dtype, kw.get("device", "cpu"), band, band, None, pattern, 256)
            arenas.append(a)
            return a.view
        return _byte_fill(real.empty(*size, **kw), pattern)

    def empty_like(t, **kw):
        kw.setdefault("dtype", t.dtype)
        kw.setdefault("device", t.device)
        return empty(tuple(t.shape), **kw)

    proxy = _TorchProxy(real, empty, empty_like)
    n = 0
    for name, mod in list(sys.modules.items()):
        if mod is None or not (name == prefix or name.startswith(prefix + ".")):
            continue
        if getattr(mod, "torch", None) is real:
            monkeypatch.setattr(mod, "torch", proxy)
            n += 1
    assert n, "no loaded %s module imports torch at module level: nothing was patched" % prefix
    return arenas
