"""The arena of tests/abi_buffers.py on CPU tensors, and the completeness of the case table (tests/abi_cases.py): no GPU.

A write the arena cannot see, or an entry point without a row, would make tests/test_gpu_abi_buffers.py pass for nothing."""
import importlib

import numpy as np
import pytest

from . import abi_buffers as ab
from . import abi_cases as ac

SIGNATURES = importlib.import_module("3dahv_amd._lib").SIGNATURES


def arena():
    a = ab.Arena("cpu")
    a.add(ab.In("R", np.arange(3 * 18, dtype=np.float32), rows=3, stride="r"), stride=18 + ab.PAD)
    a.add(ab.In("idx", np.arange(6, dtype=np.int64), filler=ab.KEY_EMPTY))
    a.add(ab.Out("out", np.float32, 7, rows=3, stride="o"), shift=4, stride=7 + ab.PAD, prefill="nan")
    a.add(ab.InOut("keys", np.full(3, ab.KEY_EMPTY, np.int64)))
    a.add(ab.Ws("workspace", 48, "workspace_bytes"), prefill=0xFF)
    return a


def words(slot):
    return slot.dev.numpy().view(np.uint32)


def test_layout_bands_gaps_and_bases():
    a = arena()
    R, out, idx, ws = a["R"], a["out"], a["idx"], a["workspace"]
    assert R.ptr % 16 == 0 and out.ptr % 16 == 4 and ws.ptr % 16 == 0
    for s in a.slots.values():
        assert s.start >= ab.BAND and s.dev.numel() - s.mask.nonzero()[0][-1] - 1 >= ab.BAND
    # float input: NaN words in bands and gaps, the rows where the stride puts them
    w = words(R)
    first = R.start // 4
    assert (w[:first] == ab.NAN_WORD).all() and (w[first + 18:first + 18 + ab.PAD] == ab.NAN_WORD).all()
    assert np.array_equal(w[first + 23:first + 41].view(np.float32), np.arange(18, 36, dtype=np.float32))
    # integer input: a value valid for the argument; output: 0xA5 around a NaN-prefilled payload at +4 bytes
    assert (idx.dev.numpy().view(np.int64)[:ab.BAND // 8] == ab.KEY_EMPTY).all()
    o = out.dev.numpy()
    assert (o[:out.start] == ab.PATTERN).all() and (o[out.start + 28:out.start + 28 + 4 * ab.PAD] == ab.PATTERN).all()
    assert (o[out.start:out.start + 28].view(np.uint32) == ab.NAN_WORD).all()
    assert (ws.dev.numpy()[ws.start:ws.start + 48] == 0xFF).all()
    assert a.report() == [] and a.untouched()
    assert a.outputs()["out"].shape == (3, 7) and a.outputs()["keys"].dtype == np.int64


def test_a_write_one_word_past_a_payload_is_reported_by_name():
    a = arena()
    out = a["out"]
    end = out.start + (2 * (7 + ab.PAD) + 7) * 4
    out.dev.numpy()[end:end + 4] = 0
    rep = a.report()
    assert len(rep) == 1 and rep[0].startswith("out: band after the payload written (byte 0 past the end)"), rep
    assert not a.untouched()


def test_a_write_in_front_of_a_payload_is_reported_by_name():
    a = arena()
    ws = a["workspace"]
    ws.dev.numpy()[ws.start - 4:ws.start] = 0
    assert a.report() == ["workspace: band before the payload written (4 bytes in front)"]


def test_a_write_into_a_stride_gap_is_reported_by_name():
    a = arena()
    out = a["out"]
    out.dev.numpy()[out.start + 7 * 4:out.start + 8 * 4] = 0
    rep = a.report()
    assert len(rep) == 1 and rep[0].startswith("out: stride gap written (byte 28 of the payload span, behind row 0)"), rep


def test_a_write_inside_a_payload_is_no_violation():
    a = arena()
    a["out"].dev.numpy()[a["out"].start:a["out"].start + 28] = 0
    a["keys"].dev.numpy()[a["keys"].start:a["keys"].start + 8] = 1
    assert a.report() == [] and not a.untouched()


@pytest.mark.parametrize("where", ["payload", "gap", "band"])
def test_a_changed_input_is_reported_by_name(where):
    a = arena()
    R = a["R"]
    at = {"payload": R.start + 8, "gap": R.start + 18 * 4, "band": 16}[where]
    R.dev.numpy()[at] ^= 1
    rep = a.report()
    assert len(rep) == 1 and rep[0].startswith("R: input changed"), rep
    assert ("outside the payload" in rep[0]) == (where != "payload")


def test_every_entry_point_has_a_row_or_a_stated_exemption():
    rows, exempt = set(ac.ROWS), set(ac.EXEMPT)
    assert set(SIGNATURES) - rows - exempt == set()
    assert rows | exempt <= set(SIGNATURES), "a row for an entry point that does not exist"
    assert not rows & exempt and all(ac.EXEMPT.values())


@pytest.mark.parametrize("entry", sorted(ac.ROWS))
def test_a_row_declares_the_pointers_of_its_signature(entry):
    argtypes = SIGNATURES[entry][1]
    for case in ac.cases(entry):
        assert case.entry == entry
        assert len(case.args) + 1 == len(argtypes), (case.name, len(case.args) + 1, len(argtypes))
        import ctypes
        n_ptr = sum(t is ctypes.c_void_p for t in argtypes)
        assert case.pointer_count() == n_ptr, (case.name, case.pointer_count(), n_ptr)
        for st in case.strides():
            assert [p for p in case.ptrs() if p.stride == st.name], st.name
        for a in case.args:
            if isinstance(a, ab.Size):
                assert {p.name: p for p in case.ptrs()}[a.of].role in ("ws", "inout")     # inout: a workspace that carries a state
