"""The raw C ABI (include/ahv.h) on guarded buffers: one sweep per entry point over the cases of tests/abi_cases.py, through
ctypes, by the variants of tests/abi_buffers.py::sweep --

  baseline        packed strides, aligned bases, zero-filled outputs and a workspace of exactly *_workspace_bytes(): the bytes
                  equal what the ops.py wrapper returns, and are finite, not constant and different between samples;
  bounds          in every variant all bands and stride gaps of outputs, workspaces and states are intact and every input
                  is byte-identical afterwards;
  padded strides  each *_batch_stride = packed + 5 floats: the baseline's bytes where the header accepts >=, AHV_EINVAL
                  naming the argument and nothing launched where it demands the packed value;
  dirty buffers   outputs and workspaces pre-filled with 0xFF and with NaN words: the same bytes;
  workspace size  sixteen bytes fewer than asked: AHV_EINVAL, nothing launched;
  alignment       every 4-byte-typed pointer without a stated alignment at +4 bytes: the baseline's bytes, or AHV_EINVAL
                  naming the argument where a kernel reads it through a vector type.

The three entries that sum with float atomics are held, in every variant, to their fp64 references instead of to the
baseline's bits: ahv_rotate_volume_backward_f32 to the fp64 adjoint under the rule of tests/oplevel_cases.py (e_got <= MARGIN
e_ref), ahv_score_hypotheses_backward_f32 and ..._saved_f32 to tests/test_gpu_backward.py's KinkReference at its GRAD_RTOL.

Checked against deliberately wrong builds (not kept; each defect stays inside the arena):
 (a) select_topk_kernel forming a sample's row as R + b*N*9 instead of R + b*r_batch_stride: fails ahv_select_rotation_f32 and
     ahv_select_topk_f32 here ("r_batch_stride padded: R_out differ from the baseline", every N, with and without the key reset)
     and nothing else; all 114 tests of tests/test_gpu_topk.py, test_gpu_modes.py, test_gpu_select_bytes.py and
     test_gpu_verify.py pass with it: no existing test passes a stride with a gap.
 (b) fuse_views_kernel storing its float4 without the n0 + 3 < N test: fails ahv_fuse_view_scores_f32 here in the N = 6 case
     ("fused: band after the payload written (byte 0 past the end)", in every variant).  N = 5 and N = 1025 alone do NOT
     notice it: with B = 3 and N % 4 = 1 only row 0 ends on a 16-byte boundary, its stray store lands in row 1's first floats
     and row 1's own workgroup writes them again; N = 6 is in the table because there the LAST row does.  Of the existing suite
     tests/test_gpu_views.py (4 cases of test_fuse_against_the_reference), tests/test_gpu_views_compact.py (8) and
     tests/test_gpu_track_views.py (4) also fail: they see wrong values, not the bytes past the end.
 (c) the zero fill of grad_W2 taken out of the scorer's backward (an OUTPUT, not a workspace: see (d) for one): fails
     ahv_score_hypotheses_backward_f32 and ..._saved_f32 here in both dirty-output variants (grad_W2 is NaN) and passes the zero-filled baseline; 30 tests of
     tests/test_gpu_backward.py and tests/test_gpu_graph_replay.py's forward-backward replay fail as well (torch.empty hands
     them used memory).
 (d) a workspace dependence: round 0 of topk_modes_kernel writing only the existing slots of its alive state, so that the
     padding of a row (N rounded up to 4) keeps what the workspace held.  Fails ahv_topk_modes_f32 and ahv_topk_modes_sym_f32
     here: "prefill 255 / prefill nan: keys differ from the baseline" at N = 5, 6 and 1025 (a NaN-word padding slot is a
     large key and is listed), and at N = 5 and 6 the zero-filled baseline no longer equals the ops wrapper's keys, whose
     workspace is used memory.  Of the existing suite 3 tests of tests/test_gpu_modes.py and 8 of tests/test_gpu_sym.py fail
     too.  The workspace of ahv_score_hypotheses_backward_saved_f32 is a state the training forward leaves and is
     therefore never dirtied: no variant here shows a dependence of that entry on workspace bytes outside that state.
Each row also passes every batch stride one element short of the packed row (AHV_EINVAL naming it, nothing launched).
"""
import pytest
import torch

from . import abi_buffers as ab
from . import abi_cases as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(ahv):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ahv._lib.load()


@pytest.mark.parametrize("entry", sorted(ac.ROWS))
def test_entry_point_keeps_to_its_buffers(ahv, lib, entry):
    dev = torch.device("cuda:0")
    sizes = lambda name, *a: int(getattr(lib, name)(*a))
    sizes.live = True          # a row may run the library to prepare a carried state
    bad = []
    for case in ac.cases(entry, sizes, lib.ahv_device_cu_count()):
        bad += ab.sweep(lib, ahv.ops, case, dev)
    assert not bad, "\n" + "\n".join(bad)
