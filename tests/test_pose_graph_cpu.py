"""Joint pose inference over an unposed image set, CPU tier: argument validation of ``ahv_pose_graph_init_f32`` /
``ahv_pose_graph_propose_f32`` / ``ahv_pose_graph_commit_f32`` through the ctypes table (validation runs before any HIP call),
the host-side checks of the ops and of ``posegraph.PoseGraph``, the numpy reference's own rules
(tests/pose_graph_reference.py), ``PoseGraph``'s control flow and ``harness.solve_views`` on an oracle-backed backend, and the
planted graph."""
import os
import re

import numpy as np
import pytest
import torch

from . import pose_graph_reference as pgr
from . import track_reference as tr
from .conftest import REPO

NAMES = ("ahv_pose_graph_init_f32", "ahv_pose_graph_propose_f32", "ahv_pose_graph_commit_f32")


@pytest.fixture(scope="module")
def lib(ahv):
    ahv._lib.build()
    return ahv._lib.load()


def _head(g128):
    T = lambda k: torch.from_numpy(np.ascontiguousarray(g128[k]))
    return T("W1"), T("W2"), T("b2")


# ---- 1. the entry points refuse bad arguments before any HIP call ---------------------------------------------------
def _refusals(lib, f, ok, prefix):
    def refused(word, **kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        assert f(*a) == -1, kw
        msg = lib.ahv_last_error()
        assert msg.startswith(prefix) and word in msg, (kw, msg)
    return refused


def test_pose_graph_init_argument_validation_needs_no_gpu(lib, ahv):
    # (pair_R, pair_score, edges, B, V, E, root, A, parent_edge, reached, stream)
    refused = _refusals(lib, lib.ahv_pose_graph_init_f32, [16, 16, 16, 2, 4, 12, 0, 16, 16, 16, None], b"pose_graph_init")
    for i in (0, 1, 2, 7, 8, 9):
        refused(b"null", **{"_%d" % i: None})
    refused(b"V =", _4=1)
    refused(b"V =", _4=ahv._lib.AHV_GRAPH_MAX_NODES + 1)
    refused(b"E =", _5=0)
    refused(b"E =", _5=ahv._lib.AHV_GRAPH_MAX_EDGES + 1)
    refused(b"root =", _6=4)
    refused(b"root =", _6=-1)
    refused(b"B =", _3=0)
    refused(b"B =", _3=65536)


def test_pose_graph_propose_argument_validation_needs_no_gpu(lib, ahv):
    # (A, pair_R, pair_score, edges, incident, B, V, E, k, D, N, n_fresh, seed, counter, sweep, sigma_rad, Q, Rrel, stream)
    ok = [16, 16, 16, 16, 16, 2, 4, 12, 1, 6, 64, 4, 0, None, 0, 0.1, 16, 16, None]
    refused = _refusals(lib, lib.ahv_pose_graph_propose_f32, ok, b"pose_graph_propose")
    for i in (0, 1, 2, 3, 4, 16, 17):
        refused(b"null", **{"_%d" % i: None})
    refused(b"V =", _6=17)
    refused(b"E =", _7=0)
    refused(b"k =", _8=4)
    refused(b"D =", _9=0)
    refused(b"D =", _9=ahv._lib.AHV_VIEWS_MAX + 1)
    refused(b"1 + D + n_fresh", _10=10)            # 1 + 6 + 4 = 11 slots
    refused(b"1 + D + n_fresh", _11=58)
    refused(b"n_fresh", _11=-1)
    refused(b"2^31", _10=1 << 31)
    refused(b"sweep", _14=256)
    refused(b"sweep", _14=-1)
    refused(b"sigma", _15=-0.5)
    refused(b"sigma", _15=float("nan"))
    refused(b"sigma", _15=float("inf"))
    refused(b"B =", _5=0)


def test_pose_graph_commit_argument_validation_needs_no_gpu(lib):
    # (key, Q, B, V, k, N, A, node_score, stream)
    refused = _refusals(lib, lib.ahv_pose_graph_commit_f32, [16, 16, 2, 4, 1, 64, 16, 16, None], b"pose_graph_commit")
    for i in (0, 1, 6, 7):
        refused(b"null", **{"_%d" % i: None})
    refused(b"V =", _3=1)
    refused(b"k =", _4=4)
    refused(b"N =", _5=0)
    refused(b"N =", _5=1 << 31)
    refused(b"B =", _2=65536)


def test_abi_version_unchanged_and_prototypes_agree(lib, ahv):
    assert lib.ahv_abi_version() == (2 << 16) | 3
    text = open(os.path.join(REPO, "include", "ahv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        proto = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(proto.split(",")) == len(ahv._lib.SIGNATURES[name][1]), name
    assert ahv._lib.AHV_GRAPH_MAX_NODES == int(re.search(r"#define AHV_GRAPH_MAX_NODES (\d+)", text).group(1))
    assert ahv._lib.AHV_GRAPH_MAX_EDGES == int(re.search(r"#define AHV_GRAPH_MAX_EDGES (\d+)", text).group(1))
    assert ahv._lib.AHV_GRAPH_EDGE_OUTGOING == 1 << int(re.search(r"#define AHV_GRAPH_EDGE_OUTGOING \(1 << (\d+)\)", text).group(1))
    assert pgr.OUTGOING == ahv._lib.AHV_GRAPH_EDGE_OUTGOING


# ---- 2. the ops and PoseGraph check on the host ---------------------------------------------------------------------------
def test_topology_refusals_and_layout(ahv):
    ops = ahv.ops
    with pytest.raises(RuntimeError, match="degree 18"):
        ops.PoseGraphTopology(10)                                   # complete ordered graph: degree 2 (V - 1)
    assert max(ops.PoseGraphTopology(9).degree) == 16
    with pytest.raises(RuntimeError, match="names a node outside"):
        ops.PoseGraphTopology(3, [(0, 1), (1, 3)])
    with pytest.raises(RuntimeError, match="names a node outside"):
        ops.PoseGraphTopology(3, [(0, 1), (-1, 2)])
    with pytest.raises(RuntimeError, match="self-loop"):
        ops.PoseGraphTopology(3, [(0, 1), (2, 2)])
    with pytest.raises(RuntimeError, match="n_views"):
        ops.PoseGraphTopology(1)
    with pytest.raises(RuntimeError, match="n_views"):
        ops.PoseGraphTopology(17, [(0, 1)])
    with pytest.raises(RuntimeError, match="root"):
        ops.PoseGraphTopology(3, root=3)
    with pytest.raises(RuntimeError, match="edges"):
        ops.PoseGraphTopology(3, [])
    top = ops.PoseGraphTopology(3, [(0, 1), (2, 1), (1, 0)])
    assert top.degree == [2, 3, 1] and top.offset == [0, 2, 5]
    assert top.incident == pgr.incident(top.edges, 3)
    O = pgr.OUTGOING
    assert top.incident_dev.tolist() == [0 | O, 2, 0, 1, 2 | O, 1 | O]
    assert top.edges_dev.dtype == torch.int32 and top.edges_dev.tolist() == [[0, 1], [2, 1], [1, 0]]


def test_ops_check_arguments_before_any_launch(ahv):
    ops = ahv.ops
    top = ops.PoseGraphTopology(3)
    B, E, V = 2, 6, 3
    P, s = torch.eye(3).repeat(B, E, 1, 1), torch.zeros(B, E)
    A, ns = torch.eye(3).repeat(B, V, 1, 1), torch.zeros(B, V)
    key, Q = torch.zeros(B, dtype=torch.int64), torch.eye(3).repeat(B, 8, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pose_graph_init(P, s, top)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pose_graph_propose(A, P, s, top, 1, 8, 3.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pose_graph_commit(key, Q, A, ns, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v = torch.zeros(B, 4, 16, 8, 8, 8)
        ops.pose_graph_score(v, v, torch.eye(3).repeat(B, 4, 8, 1, 1), torch.zeros(32, 384), torch.zeros(32, 32), torch.zeros(32))
    with pytest.raises(RuntimeError, match="pair_R must be"):
        ops.pose_graph_init(P[:, :5], s, top)
    with pytest.raises(RuntimeError, match="pair_score must be"):
        ops.pose_graph_init(P, s[:1], top)
    with pytest.raises(RuntimeError, match="topology must be"):
        ops.pose_graph_init(P, s, None)
    with pytest.raises(RuntimeError, match=r"1 \+ D \+ n_fresh"):
        ops.pose_graph_propose(A, P, s, top, 1, 4, 3.0)              # D = 4: 5 slots at least
    with pytest.raises(RuntimeError, match=r"1 \+ D \+ n_fresh"):
        ops.pose_graph_propose(A, P, s, top, 1, 8, 3.0, n_fresh=4)
    with pytest.raises(RuntimeError, match="k = 3"):
        ops.pose_graph_propose(A, P, s, top, 3, 8, 3.0)
    with pytest.raises(RuntimeError, match="sweep"):
        ops.pose_graph_propose(A, P, s, top, 1, 8, 3.0, sweep=256)
    with pytest.raises(RuntimeError, match="sigma_deg"):
        ops.pose_graph_propose(A, P, s, top, 1, 8, -1.0)
    with pytest.raises(RuntimeError, match="A must be"):
        ops.pose_graph_propose(A[:, :2], P, s, top, 1, 8, 3.0)
    with pytest.raises(RuntimeError, match="no incident edge"):
        ops.pose_graph_propose(torch.eye(3).repeat(B, 4, 1, 1), P[:, :2], s[:, :2], ops.PoseGraphTopology(4, [(0, 1), (1, 2)]), 3, 8, 3.0)
    with pytest.raises(RuntimeError, match="k = 3"):
        ops.pose_graph_commit(key, Q, A, ns, 3)
    with pytest.raises(RuntimeError, match="node_score must be"):
        ops.pose_graph_commit(key, Q, A, ns[:, :2], 1)
    with pytest.raises(RuntimeError, match="Q must be"):
        ops.pose_graph_commit(key, Q[:1], A, ns, 1)
    with pytest.raises(RuntimeError, match="no autograd edge"):
        v = torch.zeros(B, 4, 16, 8, 8, 8)
        ops.pose_graph_score(v.clone().requires_grad_(), v, torch.eye(3).repeat(B, 4, 8, 1, 1), torch.zeros(32, 384),
                             torch.zeros(32, 32), torch.zeros(32))
    with pytest.raises(RuntimeError, match="vol_tgt must be"):
        v = torch.zeros(B, 4, 16, 8, 8, 8)
        ops.pose_graph_score(v, v[:, :3], torch.eye(3).repeat(B, 4, 8, 1, 1), torch.zeros(32, 384), torch.zeros(32, 32),
                             torch.zeros(32))


def test_pose_graph_constructor_refusals(ahv, oracle, g128):
    PG = ahv.posegraph.PoseGraph
    W = _head(g128)
    be = pgr.make_backend(ahv, oracle)
    with pytest.raises(RuntimeError, match="degree 18"):
        PG(*W, n_views=10, backend=be)
    with pytest.raises(RuntimeError, match=r"1 \+ D_k \+ n_fresh"):
        PG(*W, n_views=4, candidates=7, n_fresh=1, backend=be)       # D = 6: 8 slots at least
    PG(*W, n_views=4, candidates=8, n_fresh=1, backend=be)
    with pytest.raises(RuntimeError, match="names a node outside"):
        PG(*W, n_views=3, edges=[(0, 3)], backend=be)
    with pytest.raises(RuntimeError, match="self-loop"):
        PG(*W, n_views=3, edges=[(1, 1)], backend=be)
    with pytest.raises(RuntimeError, match="use_graph=True needs the HIP backend"):
        PG(*W, n_views=3, use_graph=True, backend=be)
    with pytest.raises(RuntimeError, match="use_graph=True needs the HIP backend"):
        PG(*W, n_views=3, use_graph=True)                            # weights on the CPU
    with pytest.raises(RuntimeError, match="edge_weights must hold"):
        PG(*W, n_views=3, edge_weights=[1.0], backend=be)
    with pytest.raises(RuntimeError, match="without an edge"):
        PG(*W, n_views=3, edges=[(0, 1), (1, 2)], edge_weights=[1.0, 0.0], backend=be)
    with pytest.raises(RuntimeError, match="sigma_deg"):
        PG(*W, n_views=3, sigma_deg=(3.0, -1.0), backend=be)
    with pytest.raises(RuntimeError, match="needs a backend that provides"):
        PG(*W, n_views=3, backend=tr.make_backend(ahv, oracle))
    g = PG(*W, n_views=3, backend=be)
    with pytest.raises(RuntimeError, match="vol_src must be"):
        g.solve(torch.zeros(1, 5, 16, 8, 8, 8), torch.zeros(1, 6, 16, 8, 8, 8), torch.eye(3)[None])
    with pytest.raises(RuntimeError, match="R0 must be"):
        g.solve(torch.zeros(1, 6, 16, 8, 8, 8), torch.zeros(1, 6, 16, 8, 8, 8), torch.eye(3))


# ---- 3. the reference's own rules -----------------------------------------------------------------------------------------
def test_reference_prim_is_a_maximum_spanning_tree_with_the_tie_rule():
    rng = np.random.default_rng(5)
    for V in (2, 3, 4, 5):
        edges = pgr.complete(V)
        for trial in range(6):
            s = rng.uniform(-1, 1, len(edges))
            if trial % 2 and V > 2:
                s[rng.choice(len(edges), 2, replace=False)] = [np.nan, -np.inf]
            parent, reached, order, _ = pgr.prim(s, edges, V, root=trial % V)
            best, got = pgr.best_spanning_weight(s, edges, V, root=trial % V)
            assert got == pytest.approx(best, abs=1e-12) and reached.all() and (parent >= 0).sum() == V - 1
    # exact ties go to the lower edge index; an edge of either direction joins its two nodes
    edges = [(1, 0), (0, 1), (0, 2), (2, 1)]
    parent, reached, order, gap = pgr.prim([0.5, 0.5, 0.5, 0.9], edges, 3)
    assert [e for e, _, _ in order] == [0, 3] and parent.tolist() == [-1, 0, 3] and gap == pytest.approx(0.4)
    # an isolated node and a non-finite bridge
    parent, reached, _, _ = pgr.prim([0.3, np.nan], [(0, 1), (1, 2)], 4)
    assert reached.tolist() == [1, 1, 0, 0] and parent.tolist() == [-1, 0, -1, -1]


def test_reference_propagation_and_edge_rotations_are_consistent(ahv):
    V = 5
    edges = pgr.complete(V)
    truth = pgr.planted_truth(ahv.rotations, V, 3)
    P = pgr.relative(truth, edges)
    s = np.random.default_rng(1).uniform(0, 1, len(edges))
    _, _, order, _ = pgr.prim(s, edges, V, root=2)
    A, bound = pgr.propagate(P, edges, order, V, root=2)
    assert np.allclose(pgr.relative(A, edges), P, atol=1e-12)        # exact pairs: any tree reproduces every relative rotation
    assert np.allclose(A[2], np.eye(3)) and (bound[2] == 0).all()
    inc = pgr.incident(edges, V)
    Q = pgr.candidates(A, P, s, edges, inc[1], 1, np.zeros((12, 3)))
    assert np.allclose(Q, A[1][None], atol=1e-12)                    # every neighbour implies the consistent rotation
    Rrel = pgr.edge_rotations(Q, A, edges, inc[1])
    for d, (e, _) in enumerate(inc[1]):
        assert np.allclose(Rrel[d], P[e][None], atol=1e-12)
    s2 = s.copy()
    s2[inc[1][0][0]] = np.nan
    P2 = P.copy()
    P2[inc[1][0][0]] = 0
    assert np.array_equal(pgr.candidates(A, P2, s2, edges, inc[1], 1, np.zeros((12, 3)))[1], A[1])


def test_reference_commit_skips_a_sample_without_a_finite_score(ahv):
    pack = ahv.dist.pack_keys_host
    A, ns = np.tile(np.eye(3, dtype=np.float32), (3, 2, 1, 1)), np.zeros((3, 2), np.float32)
    Q = np.random.default_rng(0).standard_normal((3, 4, 3, 3)).astype(np.float32)
    keys = pack(np.array([0.25, np.nan, 0.5], np.float32), np.array([2, 1, 3]))
    keys[2] = pgr.vr.EMPTY
    newA, news = pgr.commit(A, ns, Q, keys, 1)
    assert np.array_equal(newA[0, 1], Q[0, 2]) and news[0, 1] == np.float32(0.25)
    assert np.array_equal(newA[1:], A[1:]) and (news[1:] == 0).all() and np.array_equal(newA[:, 0], A[:, 0])


# ---- 4. PoseGraph's control flow on the oracle backend ------------------------------------------------------------------
def _small_problem(ahv, oracle, V=3, seed=0, B=1):
    rot = lambda vol, R: oracle.rotate_volume(vol, np.asarray(R, np.float32)[None])
    vs, vt, truth, bad = pgr.planted_volumes(rot, ahv.rotations, V, 0, seed)
    R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(96, seed=31))
    vs, vt = torch.from_numpy(vs).repeat(B, 1, 1, 1, 1, 1), torch.from_numpy(vt).repeat(B, 1, 1, 1, 1, 1)
    return vs, vt, R0, truth


def test_pose_graph_control_flow_on_the_oracle_backend(ahv, oracle, g128):
    W = _head(g128)
    vs, vt, R0, _ = _small_problem(ahv, oracle, V=3, B=2)
    be = pgr.make_backend(ahv, oracle)
    g = ahv.posegraph.PoseGraph(*W, n_views=3, batch=2, candidates=16, sweeps=2, sigma_deg=(4, 2), root=1, seed=5, backend=be)
    res = g.solve(vs, vt, R0)
    update = lambda k: ["pose_graph_propose:%d" % k, "pose_graph_score", "pose_graph_commit:%d" % k]
    # E = 6 <= 16: one gather per node and tensor; the root (1) is never proposed for or committed
    assert be.calls == (["verify_pair", "select_rotation", "track_advance", "pose_graph_init"] + ["gather_views"] * 4
                        + (update(0) + update(2)) * 2)
    assert int(g.counter[0]) == 1
    eye = torch.eye(3).expand(2, 3, 3)
    assert torch.equal(res.A[:, 1], eye) and torch.equal(res.init_A[:, 1], eye) and torch.isnan(res.node_score[:, 1]).all()
    assert torch.isfinite(res.node_score[:, [0, 2]]).all()
    # init_A is the reference tree of the pairwise arg-maxes
    for b in range(2):
        parent, reached, order, _ = pgr.prim(res.pair_score[b].numpy(), g.topology.edges, 3, root=1)
        A, _ = pgr.propagate(res.pair_R[b].numpy(), g.topology.edges, order, 3, root=1)
        assert np.array_equal(res.init_A[b].numpy(), A.astype(np.float32))
        assert np.array_equal(res.parent_edge[b].numpy(), parent) and np.array_equal(res.reached[b].numpy(), reached)
    assert torch.equal(res.init_A[0], res.init_A[1])                              # two samples of one problem, their own noise
    first = res.A.clone()
    # the staged lists are the incident edges' volumes
    for k in (0, 2):
        ids = [e for e, _ in g.topology.incident[k]]
        assert torch.equal(g._staged[k][0], vs[:, ids]) and torch.equal(g._staged[k][1], vt[:, ids])
    # same seed and counter: the same bytes; a second solve of one object (counter 2) or another seed: other bytes
    again = ahv.posegraph.PoseGraph(*W, n_views=3, batch=2, candidates=16, sweeps=2, sigma_deg=(4, 2), root=1, seed=5,
                                    backend=pgr.make_backend(ahv, oracle)).solve(vs, vt, R0)
    assert torch.equal(again.A, first) and torch.equal(again.init_A, res.init_A)
    other = ahv.posegraph.PoseGraph(*W, n_views=3, batch=2, candidates=16, sweeps=2, sigma_deg=(4, 2), root=1, seed=6,
                                    backend=pgr.make_backend(ahv, oracle)).solve(vs, vt, R0)
    assert not torch.equal(other.A, first) and torch.equal(other.init_A, res.init_A)
    second = g.solve(vs, vt, R0)
    assert int(g.counter[0]) == 2 and not torch.equal(second.A, first)
    assert torch.allclose(g.relative(), torch.from_numpy(pgr.relative(second.A.numpy(), g.topology.edges)).float(), atol=1e-6)


def test_pose_graph_stages_a_wide_edge_list_in_windows_and_honours_weights(ahv, oracle, g128):
    W = _head(g128)
    V = 5                                                                          # E = 20 > 16: windows of 16 edges per sample
    vs, vt, R0, _ = _small_problem(ahv, oracle, V=V, B=2)
    vs[1] += 1.0                                                                   # (distinct samples: a window must not mix them)
    be = pgr.make_backend(ahv, oracle)
    weights = [1.0] * 20
    weights[7] = 0.0
    g = ahv.posegraph.PoseGraph(*W, n_views=V, batch=2, candidates=12, sweeps=1, backend=be, edge_weights=weights)
    g.solve(vs, vt, R0[:32])
    for k in range(1, V):
        ids = [e for e, _ in g.topology.incident[k]]
        assert torch.equal(g._staged[k][0], vs[:, ids]) and torch.equal(g._staged[k][1], vt[:, ids])
    # edge 7 = (1, 4) weighs 0: its scores are never computed in an update of node 1 or 4
    assert g.weights[1][[e for e, _ in g.topology.incident[1]].index(7)] == 0.0
    assert (be.last_edge_scores[:, [e for e, _ in g.topology.incident[4]].index(7)] == 0).all()


def test_solve_views_on_synthetic_sequences(ahv, oracle, g128):
    W = _head(g128)
    item = next(iter(ahv.harness.SyntheticSequences(n_seq=1, n_frames=5, layer4=True, seed=3, in_channel=8)))
    vol = torch.from_numpy(np.random.default_rng(2).standard_normal((5, 16, 8, 8, 8)).astype(np.float32))
    seen = []

    def encoder(src, tgt):     # a stand-in encoder: a frame's volume by its first feature value
        lookup = {float(item["layer4"][t, 0, 0, 0]): t for t in range(5)}
        ids = [(lookup[float(a[0, 0, 0])], lookup[float(b[0, 0, 0])]) for a, b in zip(src, tgt)]
        seen.append(ids)
        return vol[[i for i, _ in ids]], vol[[j for _, j in ids]]

    frames = [4, 0, 2]
    g = ahv.posegraph.PoseGraph(*W, n_views=3, candidates=12, sweeps=1, backend=pgr.make_backend(ahv, oracle))
    props = torch.from_numpy(ahv.rotations.haar_rotations_np(24, seed=3))
    out = ahv.harness.solve_views(None, item, frames, g, props, encoder_fn=encoder)
    edges = pgr.complete(3)
    assert seen[-1] == [(frames[i], frames[j]) for i, j in edges] and out["frames"] == frames
    assert out["edges"].tolist() == [list(e) for e in edges]
    R = item["R"][frames].double().numpy()
    gt = pgr.relative(R, edges)
    res = g._result
    for name, rel in (("pair_err", res.pair_R[0].numpy()), ("tree_err", pgr.relative(res.init_A[0].numpy(), edges)),
                      ("joint_err", pgr.relative(res.A[0].numpy(), edges))):
        assert out[name].shape == (6,)
        assert np.allclose(out[name].numpy(), tr.geodesic_deg(rel, gt), atol=2e-2), name
    assert torch.equal(out["A"], res.A[0]) and out["node_score"].shape == (3,) and torch.equal(out["pair_score"], res.pair_score[0])
    # row vectors: the pair of edge i -> j is encoded the other way round and the truth is R_j^T R_i
    out_r = ahv.harness.solve_views(None, item, frames, g, props, encoder_fn=encoder, row_vector_R=True)
    assert seen[-1] == [(frames[j], frames[i]) for i, j in edges]
    gt_r = pgr.relative(np.swapaxes(R, -1, -2), edges)
    assert np.allclose(out_r["pair_err"].numpy(), tr.geodesic_deg(g._result.pair_R[0].numpy(), gt_r), atol=2e-2)
    with pytest.raises(RuntimeError, match="distinct frames"):
        ahv.harness.solve_views(None, item, [0, 1], g, props, encoder_fn=encoder)
    with pytest.raises(RuntimeError, match="distinct frames"):
        ahv.harness.solve_views(None, item, [0, 1, 7], g, props, encoder_fn=encoder)


# ---- 5. the planted graph ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,n_bad,seed", [(4, 2, 0), (5, 3, 1)])
def test_planted_graph_on_the_oracle_backend(ahv, oracle, g128, V, n_bad, seed):
    """Bar 1: the joint solution's LARGEST relative-rotation error over all ordered pairs, bad edges included, is below the
    MEDIAN pairwise arg-max error over the clean edges.  Bar 2: no bad edge is a tree edge.  1 024 shared Haar hypotheses for
    the pairwise stage, 128 candidates per node update, 8 sweeps with sigma = 6, 4, 3, 2, 1.5, 1, 0.75, 0.5 degrees."""
    W = _head(g128)
    rot = lambda vol, R: oracle.rotate_volume(vol, np.asarray(R, np.float32)[None])
    vs, vt, truth, bad = pgr.planted_volumes(rot, ahv.rotations, V, n_bad, seed)
    R0 = torch.from_numpy(ahv.rotations.haar_rotations_np(1024, seed=100 + seed))
    g = ahv.posegraph.PoseGraph(*W, n_views=V, candidates=128, sweeps=8, sigma_deg=pgr.SIGMA_DEG, seed=seed,
                                backend=pgr.make_backend(ahv, oracle))
    res = g.solve(torch.from_numpy(vs), torch.from_numpy(vt), R0)
    fig = pgr.planted_figures(res.A[0].numpy(), res.pair_R[0].numpy(), res.parent_edge[0].numpy(), truth, bad, V)
    tree = pgr.planted_figures(res.init_A[0].numpy(), res.pair_R[0].numpy(), res.parent_edge[0].numpy(), truth, bad, V)
    clean = [e for e in range(V * (V - 1)) if e not in bad]
    print("planted V=%d bad=%s seed=%d: joint max %.3f median %.3f | tree max %.3f | pairwise clean median %.3f max %.3f | bad %s | "
          "scores clean min %.3f bad max %.3f" % (V, bad, seed, fig["joint_max"], fig["joint_median"], tree["joint_max"],
                                                  fig["pair_clean_median"], fig["pair_clean_max"],
                                                  ["%.1f" % x for x in fig["pair_bad"]], float(res.pair_score[0, clean].min()),
                                                  float(res.pair_score[0, bad].max())))
    assert fig["joint_max"] < fig["pair_clean_median"], fig
    assert fig["bad_in_tree"] == [], fig
