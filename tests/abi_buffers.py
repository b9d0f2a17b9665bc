"""Buffers of the raw C ABI (include/ahv.h) under guard: which bytes an entry point may read and write and which layouts it
accepts.  Shared by tests/test_abi_buffers_cpu.py (the arena itself and the completeness of the table, no GPU) and
tests/test_gpu_abi_buffers.py (one sweep per entry point).  The case table is tests/abi_cases.py.

`Arena`: every pointer argument of a call lives in a buffer of its own, [band | payload | band] with 4 KiB bands, rows
`stride` elements apart when the argument has a batch stride.
  - bands and stride gaps of outputs, workspaces and in/out states hold byte 0xA5;
  - bands and gaps of float inputs hold the quiet-NaN word 0x7FC00000: a stray read that is used poisons the result;
  - bands and gaps of integer inputs hold a value that is VALID for that argument (`filler`: index 0, the EMPTY key): a wild
    integer is an address, and nothing here may make a kernel form one;
  - the payload base sits at +0 or +4 bytes off the 16-byte grid, per argument.
After the call `report()` names every output / workspace / state whose band or gap changed and every input of which any
byte (payload, gap, band) changed.

`sweep` runs one case through the variants of the issue: baseline, padded strides, dirty outputs and workspaces, a
workspace 16 bytes short, every 4-byte-typed pointer without a stated alignment at +4 bytes.
"""
import ctypes

import numpy as np
import torch

BAND = 4096
PATTERN = 0xA5
NAN_WORD = 0x7FC00000
PAD = 5                       # floats added to a batch stride
AHV_OK, AHV_EINVAL = 0, -1
KEY_EMPTY = -(1 << 63)
DIRTY = (0x00, 0xFF, "nan")   # what pure outputs and workspaces hold before the call; the first is the baseline


# ---- argument specifications -------------------------------------------------------------------------------------------------
class Ptr:
    """One device-pointer argument.  role: in | out | inout | ws.  data: (rows, row_elems) array for in / inout (rows = 1
    unless the argument has a batch stride); out / ws give dtype and shape instead.  stride: the name of the scalar that
    carries its batch stride.  align: the alignment in bytes the header states (a pointer with align <= 4 is also run at +4
    bytes); misaligned: 'match' (the call must give the baseline's bytes) or 'refuse' (AHV_EINVAL naming the argument).
    filler: what bands and gaps of an INTEGER input hold."""

    def __init__(self, name, role, data=None, dtype=None, rows=1, row_elems=None, stride=None, align=None, misaligned="match",
                 filler=0):
        assert role in ("in", "out", "inout", "ws")
        if data is not None:
            data = np.ascontiguousarray(data)
            dtype = data.dtype
            data = data.reshape(rows, -1)
            row_elems = data.shape[1]
        self.name, self.role, self.data, self.dtype = name, role, data, np.dtype(dtype)
        self.rows, self.row_elems, self.stride, self.filler = rows, int(row_elems), stride, filler
        self.align = align if align is not None else self.dtype.itemsize
        self.misaligned = misaligned
        assert role in ("in", "inout") or data is None
        assert role not in ("in", "inout") or data is not None

    @property
    def shiftable(self):
        return self.dtype.itemsize == 4 and self.align <= 4


def In(name, data, rows=1, **kw):
    return Ptr(name, "in", data=data, rows=rows, **kw)


def InOut(name, data, rows=1, **kw):
    return Ptr(name, "inout", data=data, rows=rows, **kw)


def Out(name, dtype, row_elems, rows=1, **kw):
    return Ptr(name, "out", dtype=dtype, rows=rows, row_elems=row_elems, **kw)


class Ws(Ptr):
    """A workspace of `nbytes` (the entry's own *_workspace_bytes()); its size travels in the scalar `size`."""

    def __init__(self, name, nbytes, size, align=16):
        Ptr.__init__(self, name, "ws", dtype=np.uint8, row_elems=max(int(nbytes), 16), align=align)
        self.nbytes, self.size = int(nbytes), size


class Sc:
    """A scalar argument."""

    def __init__(self, name, value):
        self.name, self.value = name, value


class Stride(Sc):
    """The batch stride (in elements) of the pointers that name it.  rule: 'ge' (the header accepts any stride >= the packed
    row) or 'eq' (0 or exactly the packed row).  shared: pass 0 (one row for the whole batch)."""

    def __init__(self, name, rule, shared=False):
        Sc.__init__(self, name, None)
        assert rule in ("ge", "eq")
        self.rule, self.shared = rule, shared


class Size(Sc):
    """workspace_bytes of the Ws argument `of`."""

    def __init__(self, name, of):
        Sc.__init__(self, name, None)
        self.of = of


class Host(Sc):
    """A HOST float array (or None): passed as it is."""

    def __init__(self, name, values):
        Sc.__init__(self, name, None)
        self.array = None if values is None else (ctypes.c_float * len(values))(*values)

    def pointer(self):
        return None if self.array is None else ctypes.cast(self.array, ctypes.c_void_p)


class Null(Sc):
    def __init__(self, name):
        Sc.__init__(self, name, None)


class Case:
    """One call of one entry point.  args: the argument list in the order of _lib.SIGNATURES[entry], without the stream.
    vary: float outputs that must be finite, not constant and different between samples (leading dimension B).
    distinct: outputs of any type (keys, indices, states, float rows that hold -inf) that must be not constant and not the same
    in every sample, byte for byte (two samples may share an index out of five; all three sharing every byte is a dead
    output); together the two lists name every output of a row that is not constant by its contract.
    ops: f(ops module, {name: cuda tensor of every in / inout payload, packed}) -> {output name: tensor}, what the wrapper
    of 3dahv_amd/ops.py returns for the same inputs.  check: f(outputs, what) for the entries whose sums use float atomics
    (fp64 reference and tolerance of their own test file), in the place of bit equality with the baseline."""

    def __init__(self, entry, name, args, B, vary=(), ops=None, check=None, distinct=()):
        self.entry, self.name, self.args, self.B, self.vary, self.ops, self.check = entry, name, args, B, tuple(vary), ops, check
        self.distinct = tuple(distinct)

    def ptrs(self):
        return [a for a in self.args if isinstance(a, Ptr)]

    def strides(self):
        return [a for a in self.args if isinstance(a, Stride)]

    def pointer_count(self):
        return sum(isinstance(a, (Ptr, Host, Null)) for a in self.args) + 1      # + the stream


# ---- the arena ---------------------------------------------------------------------------------------------------------------
def _round16(n):
    return (n + 15) & ~15


class Slot:
    def __init__(self, spec, device, shift=0, stride=None, prefill=0x00):
        item = spec.dtype.itemsize
        assert shift in (0, 4) and (shift == 0 or item == 4)
        self.spec, self.shift = spec, shift
        self.stride = spec.row_elems if stride is None else stride
        assert self.stride >= spec.row_elems or spec.rows == 1
        span = ((spec.rows - 1) * self.stride + spec.row_elems) * item
        self.start = BAND + shift
        total = _round16(self.start + span) + BAND
        if spec.role == "in" and spec.dtype.kind == "f":
            raw = np.full(total // 4, NAN_WORD, np.uint32).view(np.uint8)
        elif spec.role == "in":
            raw = np.full(total // item, spec.filler, spec.dtype).view(np.uint8)
        else:
            raw = np.full(total, PATTERN, np.uint8)
        self.mask = np.zeros(total, bool)                       # True: payload
        for r in range(spec.rows):
            lo = self.start + r * self.stride * item
            hi = lo + spec.row_elems * item
            self.mask[lo:hi] = True
            if spec.data is not None:
                raw[lo:hi] = spec.data[r].view(np.uint8)
            elif prefill == "nan":
                raw[lo:hi] = np.full((hi - lo) // 4, NAN_WORD, np.uint32).view(np.uint8) if (hi - lo) % 4 == 0 else 0xFF
            else:
                raw[lo:hi] = prefill
        self.before = raw.copy()
        self.dev = torch.from_numpy(raw).to(device)
        if self.dev.is_cuda:
            assert self.dev.data_ptr() % 256 == 0
        self.ptr = self.dev.data_ptr() + self.start
        self._after = None

    def after(self):
        if self._after is None:
            self._after = self.dev.cpu().numpy()
        return self._after

    def payload(self):
        """The rows, packed: (rows, row_elems) of the argument's dtype."""
        a, s, item = self.after(), self.spec, self.spec.dtype.itemsize
        rows = [a[self.start + r * self.stride * item:self.start + (r * self.stride + s.row_elems) * item] for r in range(s.rows)]
        return np.stack(rows).copy().view(s.dtype)

    def problems(self):
        a, b, name, item = self.after(), self.before, self.spec.name, self.spec.dtype.itemsize
        changed = a != b
        out = []
        if self.spec.role == "in":
            if changed.any():
                where = "payload" if (changed & self.mask).any() else "outside the payload"
                out.append("%s: input changed (%s, first at byte %+d of the payload)" % (name, where, int(np.argmax(changed)) - self.start))
            return out
        outside = changed & ~self.mask
        if outside.any():
            first = int(np.argmax(outside))
            end = self.start + ((self.spec.rows - 1) * self.stride + self.spec.row_elems) * item
            if first < self.start:
                out.append("%s: band before the payload written (%d bytes in front)" % (name, self.start - first))
            elif first >= end:
                out.append("%s: band after the payload written (byte %d past the end)" % (name, first - end))
            else:
                out.append("%s: stride gap written (byte %d of the payload span, behind row %d)"
                           % (name, first - self.start, (first - self.start) // (self.stride * item)))
        return out


class Arena:
    def __init__(self, device):
        self.device, self.slots = torch.device(device), {}

    def add(self, spec, shift=0, stride=None, prefill=0x00):
        assert spec.name not in self.slots
        self.slots[spec.name] = Slot(spec, self.device, shift, stride, prefill)
        return self.slots[spec.name].ptr

    def __getitem__(self, name):
        return self.slots[name]

    def report(self):
        """Every violation, by argument name; [] when the call kept to its buffers."""
        return [p for s in self.slots.values() for p in s.problems()]

    def untouched(self):
        """No byte of any buffer changed: nothing was launched."""
        return [n for n, s in self.slots.items() if (s.after() != s.before).any()] == []

    def outputs(self):
        return {n: s.payload() for n, s in self.slots.items() if s.spec.role in ("out", "inout")}


# ---- one call ----------------------------------------------------------------------------------------------------------------
class Result:
    def __init__(self, status, message, arena):
        self.status, self.message, self.arena = status, message, arena


def run(lib, case, device, shift=(), pad=(), prefill=0x00, short_ws=False, overlap=()):
    """Call case.entry on arena buffers.  shift: names of pointers placed at +4 bytes; pad: names of Stride scalars set to
    packed + PAD; prefill: what pure outputs and workspaces hold; short_ws: pass 16 bytes fewer than the workspace needs;
    overlap: names of Stride scalars PASSED as packed - 1 (rows that would overlap: the buffers stay packed, the call must be
    refused before it reads them)."""
    device = torch.device(device)
    arena, values = Arena(device), []
    ptrs = {p.name: p for p in case.ptrs()}
    stride_of = {}
    for st in case.strides():
        users = [p for p in ptrs.values() if p.stride == st.name]
        assert users and len({p.row_elems for p in users}) == 1, st.name
        packed = users[0].row_elems
        stride_of[st.name] = (0 if st.shared else packed + (PAD if st.name in pad else 0))
        if st.shared:
            assert all(p.rows == 1 for p in users) and st.name not in pad
    for a in case.args:
        if isinstance(a, Ptr):
            stride = stride_of.get(a.stride) or None
            values.append(arena.add(a, 4 if a.name in shift else 0, stride, prefill))
        elif isinstance(a, Stride):
            values.append(stride_of[a.name] - (1 if a.name in overlap else 0))
        elif isinstance(a, Size):
            values.append(max(_nbytes(ptrs[a.of]) - (16 if short_ws else 0), 0))
        elif isinstance(a, Host):
            values.append(a.pointer())
        elif isinstance(a, Null):
            values.append(None)
        else:
            values.append(a.value)
    fn = getattr(lib, case.entry)
    if device.type == "cuda":
        with torch.cuda.device(device):
            status = fn(*values, torch.cuda.current_stream(device).cuda_stream)
            torch.cuda.synchronize(device)
    else:
        status = fn(*values, None)
    message = lib.ahv_last_error().decode("utf-8", "replace") if status < 0 else ""
    return Result(status, message, arena)


def _nbytes(p):
    return p.nbytes if isinstance(p, Ws) else p.rows * p.row_elems * p.dtype.itemsize


def inputs_on(case, device):
    """{name: packed payload of every in / inout pointer as a tensor on `device`}: what the ops wrapper is given."""
    out = {p.name: torch.from_numpy(p.data.copy()).to(device) for p in case.ptrs() if p.data is not None}
    out["_device"] = torch.device(device)
    return out


# ---- the sweep ---------------------------------------------------------------------------------------------------------------
def _same(got, want):
    return all(np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)) for k in want)


def _differs(got, want):
    return [k for k in want if not np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8))]


def sweep(lib, ops, case, device):
    """All variants of one case; returns the list of failures (strings), empty when the entry holds its contract."""
    bad, what = [], "%s[%s]" % (case.entry, case.name)

    def expect_ok(res, tag, base=None):
        if res.status != AHV_OK:
            bad.append("%s %s: status %d (%s)" % (what, tag, res.status, res.message))
            return None
        for p in res.arena.report():
            bad.append("%s %s: %s" % (what, tag, p))
        out = res.arena.outputs()
        if case.check is not None:
            try:
                case.check(out, "%s %s" % (what, tag))
            except AssertionError as e:
                bad.append("%s %s: %s" % (what, tag, e))
        elif base is not None and not _same(out, base):
            bad.append("%s %s: %s differ from the baseline" % (what, tag, ", ".join(_differs(out, base))))
        return out

    def expect_refusal(res, tag, naming):
        if res.status != AHV_EINVAL:
            bad.append("%s %s: status %d, expected AHV_EINVAL" % (what, tag, res.status))
        elif naming not in res.message:
            bad.append("%s %s: the message does not name %s: %r" % (what, tag, naming, res.message))
        if not res.arena.untouched():
            bad.append("%s %s: a refused call changed device memory" % (what, tag))

    # 1. baseline: packed strides, aligned bases, zero-filled outputs and workspace of exactly the size asked
    base = expect_ok(run(lib, case, device), "baseline")
    if base is None:
        return bad
    if case.ops is not None:
        want = case.ops(ops, inputs_on(case, device))
        for k, t in want.items():
            w = t.detach().contiguous().cpu().numpy().reshape(-1).view(np.uint8)
            if case.check is None and not np.array_equal(base[k].reshape(-1).view(np.uint8), w):
                bad.append("%s baseline: %s is not what the ops wrapper returns" % (what, k))
    for k in case.vary:
        x = base[k].reshape(case.B, -1).astype(np.float64)
        if not np.isfinite(x).all():
            bad.append("%s baseline: %s is not finite" % (what, k))
        elif (x == x.flat[0]).all():
            bad.append("%s baseline: %s is constant" % (what, k))
        elif case.B > 1 and any((x[b] == x[0]).all() for b in range(1, case.B)):
            bad.append("%s baseline: %s does not differ between samples" % (what, k))
    for k in case.distinct:
        e = np.ascontiguousarray(base[k]).reshape(-1)
        e = e.view(np.uint8).reshape(e.size, -1)                 # one row of bytes per element: a NaN equals itself here
        x = e.reshape(case.B, -1)
        if (e == e[0]).all():
            bad.append("%s baseline: %s is constant" % (what, k))
        elif case.B > 1 and all(np.array_equal(x[b], x[0]) for b in range(1, case.B)):
            bad.append("%s baseline: %s is the same in every sample" % (what, k))
    # 3. padded strides, one argument at a time
    for st in case.strides():
        if st.shared:
            continue
        res = run(lib, case, device, pad=(st.name,))
        if st.rule == "ge":
            expect_ok(res, "%s padded" % st.name, base)
        else:
            expect_refusal(res, "%s padded" % st.name, st.name)
        # one element fewer than the packed row (overlapping rows) is refused under either rule
        expect_refusal(run(lib, case, device, overlap=(st.name,)), "%s one short of the packed row" % st.name, st.name)
    # 4. dirty outputs and workspaces
    for fill in DIRTY[1:]:
        expect_ok(run(lib, case, device, prefill=fill), "prefill %s" % (fill,), base)
    # 5. a workspace 16 bytes short
    ptrs = {p.name: p for p in case.ptrs()}
    for a in case.args:
        if isinstance(a, Size) and _nbytes(ptrs[a.of]) >= 16:
            expect_refusal(run(lib, case, device, short_ws=True), "%s 16 bytes short" % a.of, "")
    # 6. base alignment
    for p in case.ptrs():
        if not p.shiftable:
            continue
        res = run(lib, case, device, shift=(p.name,))
        if p.misaligned == "match":
            expect_ok(res, "%s at +4 bytes" % p.name, base)
        else:
            expect_refusal(res, "%s at +4 bytes" % p.name, p.name)
    return bad
