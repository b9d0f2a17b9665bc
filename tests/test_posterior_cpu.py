"""Pose posterior, CPU tier: the numpy reference (tests/posterior_reference.py) against the golden InfoNCE run, its merge rule
over uneven shards, the host-side argument checks of ``ops.pose_posterior`` and of the C ABI (validation runs before any HIP
call), ``dist.all_gather_posterior`` under world-2 gloo with a numpy merge, and the header against the ctypes table."""
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from . import posterior_reference as pr
from .conftest import REPO, load_golden
from .test_dist_cpu import _free_port


@pytest.fixture(scope="module")
def lib(ahv):
    ahv._lib.build()
    return ahv._lib.load()


# ---- the reference against the golden run -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["a_", "b_"])
def test_reference_reproduces_the_infonce_loss(case):
    """G11 (tests/golden/infonce_grad.npz): scores = sim, one anchor = the ground truth, theta = ACC_THR, T = 0.1.  Bucket 0 is
    the reference's positive set exactly, and -log(mode_prob[:, 0]) its per-sample loss to the tolerance that loss has."""
    g = load_golden("infonce_grad")
    sim, R, gt, thr = g[case + "sim"], g[case + "R"], g[case + "gt"], float(g["acc_thr"])
    for b in range(len(sim)):
        bucket, margin = pr.assign(R[b], gt[b][None], pr.tau_of(thr))
        assert margin > 1e-4
        assert np.array_equal(bucket == 0, g[case + "positive"][b])
    out, _ = pr.posterior(sim, R, gt[:, None], thr, 0.1)
    loss = -np.log(out["mode_prob"][:, 0])
    assert np.all(np.abs(loss - g[case + "loss_per_sample"]) <= 1e-5)
    assert abs(loss.mean() - float(g[case + "loss"])) <= 1e-5
    assert np.all(np.abs(out["mode_prob"].sum(axis=1) + out["rest_prob"] - 1) <= 1e-12)


def test_reference_merge_rule_over_uneven_shards():
    s, R, A = pr.make_inputs(1021, 2, True, 1)
    s = s.copy()
    s[0, 7], s[1, 900] = np.nan, np.inf
    beta, tau = pr.beta_of(0.02), pr.tau_of(30.0)
    for b in range(2):
        whole, _ = pr.state_of(s[b], R[b], A[b], tau, beta)
        for cuts in ([0, 1021], [0, 400, 1021], [0, 1, 3, 200, 201, 640, 1000, 1021]):
            st = pr.empty_state(4)
            for lo, hi in zip(cuts, cuts[1:]):
                st = pr.merge(st, pr.state_of(s[b, lo:hi], R[b, lo:hi], A[b], tau, beta)[0], beta)
            assert st["n_excluded"] == whole["n_excluded"] == 1
            assert np.array_equal(st["rec"][:, 0], whole["rec"][:, 0])
            assert np.all(np.abs(st["rec"][:, 1:] - whole["rec"][:, 1:]) <= 1e-12 * np.maximum(np.abs(whole["rec"][:, 1:]), 1.0))
            a, w = pr.finish(st, beta), pr.finish(whole, beta)
            for k in ("log_z", "entropy", "mean_score", "mode_prob", "rest_prob", "mode_R_mean", "R_mean"):
                assert np.all(np.abs(np.asarray(a[k]) - np.asarray(w[k])) <= 1e-12), k
        rt = pr.from_bytes(pr.to_bytes([whole]), 4)[0]
        assert rt["n_excluded"] == whole["n_excluded"] and np.array_equal(rt["rec"], whole["rec"])


def test_reference_empty_cases():
    R = pr.haar(np.random.default_rng(3), 8)
    A = np.stack([R[0], np.zeros((3, 3), np.float32)])[None]
    out, _ = pr.posterior(np.full((1, 8), np.nan, np.float32), R, A, 150.0, 0.1)
    assert out["log_z"][0] == -np.inf and np.isnan(out["entropy"][0]) and out["n_excluded"][0] == 8
    assert np.all(out["mode_prob"] == 0) and np.all(out["mode_R_mean"] == 0) and np.all(np.isnan(out["mode_spread_deg"]))
    out, _ = pr.posterior(np.zeros((1, 8), np.float32), R, A, 150.0, 0.1)
    assert out["mode_prob"][0, 1] == 0 and np.isnan(out["mode_spread_deg"][0, 1])   # the empty slot: t = 0 >= tau, skipped
    assert abs(out["entropy"][0] - np.log(8)) <= 1e-12 and abs(out["log_z"][0] - np.log(8)) <= 1e-12


# ---- host checks ------------------------------------------------------------------------------------------------------------

def test_ops_check_arguments_before_any_launch(ahv):
    s, R = torch.zeros(2, 8), torch.eye(3)[None].repeat(8, 1, 1)
    A = torch.eye(3)[None, None].repeat(2, 4, 1, 1)
    pp = ahv.ops.pose_posterior
    for bad in (0.0, -0.1, float("nan"), float("inf"), 1e-45):       # 1e-45: 1 / T overflows fp32
        with pytest.raises(RuntimeError, match="temperature"):
            pp(s, R, bad, anchors=A, min_angle_deg=15.0)
    with pytest.raises(RuntimeError, match="K = 17"):
        pp(s, R, anchors=torch.zeros(2, 17, 3, 3), min_angle_deg=15.0)
    for bad in (0.0, 180.0, -5.0, float("nan")):
        with pytest.raises(RuntimeError, match="min_angle_deg"):
            pp(s, R, anchors=A, min_angle_deg=bad)
    with pytest.raises(RuntimeError, match="min_angle_deg"):
        pp(s, R, anchors=A)
    for bad in (torch.zeros(3, 4, 3, 3), torch.zeros(2, 4, 9), torch.zeros(4, 3, 3)):
        with pytest.raises(RuntimeError, match="anchors"):
            pp(s, R, anchors=bad, min_angle_deg=15.0)
    with pytest.raises(RuntimeError, match="R holds"):
        pp(s, R[:5], anchors=A, min_angle_deg=15.0)
    with pytest.raises(RuntimeError, match="workspace of 16 bytes"):
        pp(s, R, anchors=A, min_angle_deg=15.0, workspace=torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pp(s, R, anchors=A, min_angle_deg=15.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pp(s, R)
    stride = pr.state_stride(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ahv.ops.pose_posterior_finish(torch.zeros(2, stride, dtype=torch.uint8), 4, 0.1)
    with pytest.raises(RuntimeError, match="state must be"):
        ahv.ops.pose_posterior_finish(torch.zeros(2, stride - 8, dtype=torch.uint8), 4, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ahv.ops.merge_posterior(torch.zeros(3, 2, stride, dtype=torch.uint8), 4, 0.1)
    with pytest.raises(RuntimeError, match="K = 17"):
        ahv.ops.verify_pair_posterior(None, None, R, None, None, None, 17, 15.0)
    with pytest.raises(RuntimeError, match="temperature"):
        ahv.ops.verify_pair_posterior(None, None, R, None, None, None, 4, 15.0, temperature=0.0)
    assert ahv.ops.inverse_temperature(0.1) == float(pr.beta_of(0.1)) == float(np.float32(10.0))


def test_abi_argument_validation_needs_no_gpu(lib, ahv):
    err = lib.ahv_last_error
    sb, wb = lib.ahv_pose_posterior_state_bytes, lib.ahv_pose_posterior_workspace_bytes
    assert sb(1, 0) == 16 + 2 * 96 and sb(3, 16) == 3 * (16 + 18 * 96) == 3 * pr.state_stride(16) and sb(1, 4) % 16 == 0
    assert sb(0, 4) == 0 and sb(1, 17) == 0 and sb(1, -1) == 0
    assert wb(1, 1, 4) == sb(1, 4) and wb(3, 1024, 4) == sb(3, 4) and wb(3, 1025, 4) == 2 * sb(3, 4)
    assert wb(1, 50_000, 8) == 49 * sb(1, 8) and wb(1, 10_000_000, 8) == 63 * sb(1, 8)
    assert wb(0, 10, 4) == 0 and wb(1, 0, 4) == 0 and wb(1, 10, 17) == 0
    tau = float(pr.tau_of(15.0))
    big = 1 << 20
    # (scores, R, r_batch_stride, B, N, anchors, K, min_trace, beta, state, workspace, workspace_bytes, flags, stream)
    post = lib.ahv_pose_posterior_f32
    for bad in (17, -1):
        assert post(16, 16, 0, 1, 10, 16, bad, tau, 10.0, 16, 16, big, 1, None) == -1 and b"K" in err() and str(bad).encode() in err()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert post(16, 16, 0, 1, 10, 16, 4, tau, bad, 16, 16, big, 1, None) == -1 and b"beta" in err(), bad
    for bad in (-1.0, 3.0, float("nan")):
        assert post(16, 16, 0, 1, 10, 16, 4, bad, 10.0, 16, 16, big, 1, None) == -1 and b"min_trace" in err(), bad
    for bad in (5, 89, 91):
        assert post(16, 16, bad, 1, 10, 16, 4, tau, 10.0, 16, 16, big, 1, None) == -1 and b"r_batch_stride" in err()
    assert post(16, 16, 0, -1, 10, 16, 4, tau, 10.0, 16, 16, big, 1, None) == -1 and b"negative" in err()
    assert post(16, 16, 0, 65536, 10, 16, 4, tau, 10.0, 16, 16, big, 1, None) == -1 and b"65535" in err()
    assert post(16, 16, 0, 1, 10, 16, 4, tau, 10.0, 16, 16, big, 2, None) == -1 and b"flags" in err()
    assert post(None, 16, 0, 1, 10, 16, 4, tau, 10.0, 16, 16, big, 1, None) == -1 and b"null" in err()
    assert post(16, 16, 0, 1, 10, None, 4, tau, 10.0, 16, 16, big, 1, None) == -1 and b"null" in err()
    assert post(16, 16, 0, 1, 10, 16, 4, tau, 10.0, None, 16, big, 1, None) == -1 and b"null" in err()
    assert post(16, 16, 0, 1, 10, 16, 4, tau, 10.0, 24, 16, big, 1, None) == -1 and b"aligned" in err()
    assert post(16, 16, 0, 1, 10, 16, 4, tau, 10.0, 16, None, 0, 1, None) == -1 and b"workspace" in err()
    assert post(16, 16, 0, 1, 10, 16, 4, tau, 10.0, 16, 16, sb(1, 4) - 1, 1, None) == -1 and b"workspace" in err()
    assert post(16, 16, 0, 1, 10, 16, 4, tau, 10.0, 16, 24, big, 1, None) == -1 and b"aligned" in err()
    assert post(None, None, 0, 0, 10, None, 4, tau, 10.0, None, None, 0, 1, None) == 0        # B = 0: nothing to do
    assert post(None, None, 0, 1, 0, None, 4, tau, 10.0, 16, None, 0, 0, None) == 0           # N = 0, no reset: the state stays
    # (states, P, B, K, beta, state, flags, stream)
    merge = lib.ahv_pose_posterior_merge
    assert merge(16, 2, 1, 17, 10.0, 16, 0, None) == -1 and b"K" in err()
    assert merge(16, -1, 1, 4, 10.0, 16, 0, None) == -1 and b"negative" in err()
    assert merge(16, 2, 1, 4, 0.0, 16, 0, None) == -1 and b"beta" in err()
    assert merge(None, 2, 1, 4, 10.0, 16, 0, None) == -1 and b"null" in err()
    assert merge(16, 2, 1, 4, 10.0, 16, 4, None) == -1 and b"flags" in err()
    assert merge(None, 0, 1, 4, 10.0, 16, 0, None) == 0 and merge(None, 2, 0, 4, 10.0, None, 0, None) == 0
    # (state, B, K, beta, ten outputs, stream)
    fin = lib.ahv_pose_posterior_finish_f32
    outs = [None] * 10
    assert fin(16, 1, 17, 10.0, *outs, None) == -1 and b"K" in err()
    assert fin(16, 1, 4, float("nan"), *outs, None) == -1 and b"beta" in err()
    assert fin(None, 1, 4, 10.0, *outs, None) == -1 and b"null" in err()
    assert fin(8, 1, 4, 10.0, *outs, None) == -1 and b"aligned" in err()
    assert fin(None, 0, 4, 10.0, *outs, None) == 0
    assert lib.ahv_abi_version() == (2 << 16) | 3   # added under 2.3: callers probe for the symbol


def test_header_and_ctypes_table_agree_on_the_new_prototypes(ahv):
    import ctypes
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ahv.h")).read(), flags=re.S)
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
             "unsigned": ctypes.c_uint}
    names = ["ahv_pose_posterior_state_bytes", "ahv_pose_posterior_workspace_bytes", "ahv_pose_posterior_f32",
             "ahv_pose_posterior_merge", "ahv_pose_posterior_finish_f32"]
    for name in names:
        m = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        want_args = [ctypes.c_void_p if "*" in a else kinds[a.split()[-2]] for a in (x.strip() for x in m.group(2).split(","))]
        res, args = ahv._lib.SIGNATURES[name]
        assert res is kinds[m.group(1)] and args == want_args, name
    assert ahv._lib.AHV_POSTERIOR_MAX_MODES == int(re.search(r"#define AHV_POSTERIOR_MAX_MODES (\d+)", text).group(1)) == 16
    assert ahv._lib.AHV_POSTERIOR_RESET_STATE == int(re.search(r"#define AHV_POSTERIOR_RESET_STATE (\d+)u", text).group(1))


# ---- the gather under gloo ------------------------------------------------------------------------------------------------

def _numpy_merge(states, k, temperature):
    """A merge_fn: (world, B, stride) uint8 -> (B, stride), the reference's rule in rank order."""
    beta = pr.beta_of(temperature)
    parts = [pr.from_bytes(p.numpy(), k) for p in states]
    out = []
    for b in range(states.shape[1]):
        st = pr.empty_state(k)
        for p in parts:
            st = pr.merge(st, p[b], beta)
        out.append(st)
    return torch.from_numpy(pr.to_bytes(out))


def _worker(rank, world, port, q):
    import importlib
    import sys
    sys.path.insert(0, REPO)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ahv = importlib.import_module("3dahv_amd")
        s, R, A = pr.make_inputs(1021, 3, False, 0)
        lo, hi = ahv.dist.shard_range(1021, rank, world)
        mine, _ = pr.batch_states(s[:, lo:hi], R[lo:hi], A, 30.0, 0.1)       # this rank's shard against the shared anchors
        calls = []
        real = dist.all_gather_into_tensor
        dist.all_gather_into_tensor = lambda o, t, *a, **k: (calls.append(tuple(t.shape)), real(o, t, *a, **k))[1]
        try:
            merged = ahv.dist.all_gather_posterior(torch.from_numpy(pr.to_bytes(mine)), 4, 0.1, merge_fn=_numpy_merge)
        finally:
            dist.all_gather_into_tensor = real
        assert calls == [(3, pr.state_stride(4))], calls                      # ONE exchange, of the state bytes
        q.put((rank, merged.numpy()))
    finally:
        dist.destroy_process_group()


def test_all_gather_posterior_world2(ahv):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert np.array_equal(got[0][1], got[1][1])                               # the same merged state on every rank
    s, R, A = pr.make_inputs(1021, 3, False, 0)
    want, _ = pr.posterior(s, R, A, 30.0, 0.1)
    have = pr.stack([pr.finish(st, pr.beta_of(0.1)) for st in pr.from_bytes(got[0][1], 4)])
    for k in ("log_z", "entropy", "mean_score", "mode_prob", "rest_prob", "mode_R_mean", "R_mean", "mode_spread_deg"):
        assert np.all(np.abs(have[k] - want[k]) <= 1e-9), k
    assert np.array_equal(have["n_excluded"], want["n_excluded"])
    # without a process group the state comes back as it is
    st = torch.zeros(3, pr.state_stride(4), dtype=torch.uint8)
    assert ahv.dist.all_gather_posterior(st, 4, 0.1) is st
