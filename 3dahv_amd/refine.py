"""Coarse-to-fine verification captured as ONE hipGraph (BASELINE.json configs[4]).

Build-defined: the reference scores one flat set of 50 000 random rotations
(test_objaverse.py:17, modules/model.py:184).  Here stage 1 scores N1 coarse hypotheses, stage 2
scores N2 refinements ``R* @ D[n]`` around each sample's stage-1 winner, where ``D`` is a fixed set of
small rotations (``rotations.refine_rotations(I, N2, max_angle)``; D[0] = I, so stage 2 can never
score below stage 1).  Everything between the two stages stays on the device: the winner index is
decoded from the packed key by ``ahv_compose_rotations_f32``; no host round trip, so the whole step
(2 fused scorer launches -- the first builds the target features in-launch --, compose, 2 selects) replays from a graph.
On one rank the step also exists as ONE launch (``fused=True``: ``ahv_coarse_to_fine_f32``, the workgroups meet at a
device-wide counter between the stages).

Multi-rank (one process per GPU): both hypothesis sets are sharded contiguously (``dist.shard_range``);
each stage ends in the 8*B-byte packed-key all-reduce(max) (int64 MAX on the key as the kernel packs it) -- two collectives per
step; the winner's rotation row needs no exchange (every rank composes the full refinement set of the
winner).  The verify semantics per stage
are those of modules/model.py:183-196.  With the ``nccl`` backend (= RCCL) the collectives are enqueued on
the capturing stream like any kernel, so the two stages AND their all-reduces replay from one hipGraph
(SURVEY.md section 8(d) cfg 5); other backends (gloo rehearsals, CPU tests) run the step eagerly.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.distributed as dist

from . import ops
from .dist import KEY_EMPTY, all_gather_scores, all_gather_topk, shard_range
from .rotations import refine_rotations


class CoarseToFine:
    """``backend`` provides ``verify_pair, score_hypotheses, compose_rotations, select_rotation`` with the signatures of
    ``3dahv_amd.ops`` (the default and the only product backend: HIP kernels, no CPU path); CPU tests inject an
    oracle-backed object to execute the multi-rank control flow under gloo.

    One step = FIVE launches: the coarse stage as one ``verify_pair`` launch (the target features are built inside it and
    kept for the fine stage), ``compose_rotations``, the fine stage, and one ``select_rotation`` per stage, each of which
    also hands its key back empty for the next step (no clearing launches).
    ``fused=True`` (one rank, no collectives, the HIP backend): the step is ONE launch, ``ops.coarse_to_fine`` -- both
    stages, a device-wide meeting point between them and the decoding of both keys inside ``ahv_coarse_to_fine_f32``.
    Same results bit for bit; measured 1.5 % faster (189.7 against 192.6 us for 10 000 + 1 000 hypotheses: the queue
    already hides the launches it removes), and its meeting point assumes nothing else holds compute units for long --
    hence opt-in.
    Scores do not depend on how the hypothesis sets are split over ranks, bit for bit (a team's score is a lone wave's);
    ``no_teams`` is the scheduling knob of ``ops.score_hypotheses``.  ``check()`` (host sync) raises if a one-launch step
    had to give its meeting point up -- such a step's outputs are poisoned (NaN, -1), never plausible.
    ``seeds=K > 1`` (multi-seed refinement): stage 2 refines around the K best coarse hypotheses instead of the winner alone,
    so a coarse winner in the wrong basin no longer decides the step.  The coarse stage keeps its scores, ``topk`` builds this
    rank's K-list, ``dist.all_gather_topk`` (an all-gather of 8*B*K bytes per rank + ``merge_topk``) takes the place of the
    coarse key all-reduce, every rank composes all K*N2 refinements (``compose_rotations_topk``) and scores its contiguous
    slice of that axis; the fine key all-reduce and ``select_rotation`` are today's.  Still two collectives per step.  The
    fine index lies in ``[0, K*N2)``: seed ``idx // N2`` (rank in the coarse list), refinement ``idx % N2``; the coarse
    score / index returned are the list's first entry (the arg-max) and ``self.last["coarse_topk"] = (scores, idx)``, both
    (B,K).  Seed 0's refinements are the single-seed step's, score for score, so the fine score never falls below it.
    ``seeds=1`` is the step described above, unchanged.  The one-launch kernel is not extended: ``fused`` with
    ``seeds > 1`` raises.
    ``modes=K`` with ``mode_angle_deg=theta`` (mode-seeded refinement): the K seeds are the K best DISTINCT coarse poses --
    ``ops.topk_modes``: the K-best order with every hypothesis within theta of an earlier seed left out -- instead of the K
    largest scores, which neighbours of one peak fill.  The step is the multi-seed one with that selection in its place.
    Modes do not compose across shards, so a multi-rank step gathers the coarse scores (``dist.all_gather_scores``,
    4*B*N1/world bytes per rank, in place of the list all-gather) and every rank selects over the whole row: the same list
    bit for bit however N1 was cut.  Fewer than K modes: the list ends in EMPTY slots; their refinement blocks are composed
    around row 0 to stay in bounds and scored, but take no part in any result.  ``self.last["modes"] = (scores, idx, R)``,
    (B,K), (B,K), (B,K,3,3): each mode's own best refinement, ``idx`` inside its N2-block (-inf, -1 and zeros for an EMPTY
    mode) -- ``argmax`` / ``select_rotation`` on the (B*K, N2) view of the fine scores; multi-rank, the N2-blocks are cut
    across ranks and the second all-reduce carries the (B,K) per-block keys instead of the (B,) key: still two collectives.
    The fine winner returned is the best of those (fine index ``mode * N2 + idx``), ``self.last["coarse_topk"]`` the coarse
    modes.  ``symmetry`` (a ``rotations.Symmetry`` in the source view's frame; with ``modes`` only, any other seeding raises): the
    seeds are distinct MODULO the group, so a symmetric object's K slots are not spent on copies of one pose.  With ``polish_iters > 0`` all K per-mode poses are polished (``self.last["polish"]`` is (B,K)-shaped) and the
    best polished one is returned.  ``modes=1`` gives the ``seeds=1`` step's outputs bit for bit.  Exclusive with
    ``seeds > 1`` and with ``fused``: both raise.
    ``polish_iters > 0`` (gradient-based polishing, ``ops.polish_rotations``): after the fine stage the fine winner takes
    ``polish_iters`` ascent steps on SO(3) along the rotation gradient of the score.  The fine score and ``R_pred`` returned are
    the polished ones (never below the fine winner's: an ascent step keeps the incumbent unless a candidate scores strictly
    higher), the fine index stays that of the seed, and ``self.last["polish"]`` holds ``score_before, R_before, score_after,
    R_after, theta``.  Multi-rank: after the second key all-reduce every rank holds the same winner and the whole volumes, and
    the rotation gradient is a function of the hypothesis alone bit for bit, so every rank computes the same bits -- still
    two collectives per step.  ``polish_iters=0`` is the step described above, unchanged; ``fused`` with polishing raises.
    ``resample=True`` (posterior-weighted refinement, ``ops.resample``): stage 2 scores ``M = D.shape[0]`` systematic DRAWS
    from the softmax of the coarse row at ``resample_temperature`` instead of M refinements of one winner: draw j is coarse
    hypothesis ``idx[j]`` refined by ``D[j]``, so a peak that holds 70 % of the posterior mass gets 70 % of the refinements and
    three broad peaks share them.  ``resample_u``: the offset in [0, 1) of the draws -- a float, a float32 tensor (B,) on the
    device (read there: a captured step follows it), or None for 0.5.  Slot 0 of the draw list is overwritten with the coarse
    arg-max index (one small device copy); D[0] = I, so the fine score never falls below the coarse one, as in every other
    mode of the step.  The coarse stage keeps its scores; ``compose_rotations_indexed`` takes ``compose_rotations``'s place.
    Resampling does not compose across shards (a prefix needs the whole row), so a multi-rank step follows the modes pattern:
    ``dist.all_gather_scores``, every rank resamples the whole row (the same draw list, byte for byte), takes the coarse
    arg-max from the gathered row locally, composes all M draws and scores its slice; then the fine key all-reduce -- two
    collectives per step.  ``self.last["resample"]`` is the draw list (B, M); the fine index returned lies in [0, M): the
    coarse hypothesis is ``self.last["resample"][b, idx]``.  ``polish_iters`` composes unchanged.  Exclusive with ``seeds > 1``,
    with ``modes`` and with ``fused``: each raises.  ``resample=False`` is every step described above, unchanged.
    ``use_graph``: None = captured when the step carries collectives, eager otherwise (see __init__); ``run_many`` replays
    several steps from one graph."""

    def __init__(self, W1: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor, R_coarse: torch.Tensor,
                 D: Optional[torch.Tensor] = None, n_fine: int = 1000, max_angle_deg: float = 10.0,
                 batch: int = 1, use_graph: Optional[bool] = None, group=None, seed: int = 0, backend=None,
                 want_scores: bool = False, force_collectives: bool = False, no_teams: bool = False,
                 fused: Optional[bool] = None, seeds: int = 1, polish_iters: int = 0, polish_angle_deg: float = 2.0,
                 polish_ladder=(0.25, 0.5, 1.0, 2.0), modes: int = 0, mode_angle_deg: float = 15.0, resample: bool = False,
                 resample_temperature: float = 0.1, resample_u=None, symmetry=None):
        dev = R_coarse.device
        self.ops = ops if backend is None else backend
        self.W1, self.W2, self.b2 = W1, W2, b2
        self.R_coarse = R_coarse.contiguous()
        if D is None:
            g = torch.Generator(device="cpu").manual_seed(seed)
            D = refine_rotations(torch.eye(3), n_fine, max_angle_deg, generator=g)
        self.D = D.to(dev).contiguous()
        self.B = batch
        self.group = group
        self.want_scores = want_scores
        self.no_teams = no_teams
        inited = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if inited else 1
        self.rank = dist.get_rank(group) if inited else 0
        # a 1-rank RCCL group with force_collectives exercises "collectives inside the captured graph" on one GPU
        self.collectives = self.world > 1 or (force_collectives and inited)
        self.seeds = int(seeds)
        if not 1 <= self.seeds <= 64:
            raise RuntimeError("seeds = %d outside 1..64" % self.seeds)
        if self.seeds > self.R_coarse.shape[-3]:
            raise RuntimeError("seeds = %d exceeds the %d coarse hypotheses" % (self.seeds, self.R_coarse.shape[-3]))
        if self.seeds > 1 and fused:
            raise RuntimeError("the one-launch step (fused=True) refines around ONE seed; seeds = %d needs fused=False"
                               % self.seeds)
        self.modes = int(modes)
        self.symmetry = symmetry
        if symmetry is not None and not self.modes:
            raise RuntimeError("symmetry selects the stage-2 seeds modulo the group: it needs modes = K (seeds, resample and the "
                               "one-launch step know no symmetry)")
        if self.modes:
            if not 1 <= self.modes <= 64:
                raise RuntimeError("modes = %d outside 1..64" % self.modes)
            if self.seeds > 1:
                raise RuntimeError("modes = %d and seeds = %d are two selections of the stage-2 seeds: pass one of them"
                                   % (self.modes, self.seeds))
            if fused:
                raise RuntimeError("the one-launch step (fused=True) refines around ONE seed; modes = %d needs fused=False"
                                   % self.modes)
            self.mode_angle_deg = float(mode_angle_deg)
            ops.min_trace(self.mode_angle_deg)   # raises outside (0, 180)
            self.seeds = self.modes              # the stage-2 layout is the multi-seed one: K blocks of N2
        self.resample = bool(resample)
        if self.resample:
            if self.modes:   # (first: modes = K has set seeds = K)
                raise RuntimeError("resample = True and modes = %d are two selections of the stage-2 seeds: pass one of them"
                                   % self.modes)
            if self.seeds > 1:
                raise RuntimeError("resample = True and seeds = %d are two selections of the stage-2 seeds: pass one of them"
                                   % self.seeds)
            if fused:
                raise RuntimeError("the one-launch step (fused=True) refines around ONE seed; resample = True needs fused=False")
            self.resample_temperature = float(resample_temperature)
            ops.inverse_temperature(self.resample_temperature)   # raises unless finite and > 0
            if resample_u is not None and not isinstance(resample_u, torch.Tensor):
                u = float(resample_u)
                if not 0.0 <= u < 1.0:
                    raise RuntimeError("resample_u = %r outside [0, 1)" % (resample_u,))
                resample_u = torch.full((batch,), u, dtype=torch.float32, device=dev)
            if resample_u is not None and (resample_u.dtype != torch.float32 or tuple(resample_u.shape) != (batch,)):
                raise RuntimeError("resample_u must be a float, or a float32 tensor (B,) = (%d,)" % batch)
            self.resample_u = resample_u
        self.polish_iters = int(polish_iters)
        if self.polish_iters < 0:
            raise RuntimeError("polish_iters must be >= 0")
        if self.polish_iters > 0 and fused:
            raise RuntimeError("the one-launch step (fused=True) does not polish; polish_iters = %d needs fused=False"
                               % self.polish_iters)
        self.polish_angle_deg, self.polish_ladder = float(polish_angle_deg), tuple(float(x) for x in polish_ladder)
        self._polish_out = {}
        if self.polish_iters > 0 and backend is None and dev.type == "cuda":
            # the ladder lives on the device from here on: the first polish of a slot may happen under graph capture
            # (run_many), where a host-to-device copy is not allowed
            self.polish_ladder = torch.tensor(self.polish_ladder, dtype=torch.float32, device=dev)
        self.c_lo, self.c_hi = shard_range(self.R_coarse.shape[0], self.rank, self.world)
        self.f_lo, self.f_hi = shard_range(self.seeds * self.D.shape[0], self.rank, self.world)
        capturable = (not self.collectives) or (inited and dist.get_backend(group) == "nccl")
        # Default (use_graph=None), from the kernel-trace timelines of profiles/r06_graph_timeline.txt: a hipGraphLaunch idles
        # the device ~9 us between two replays, plain launches none -- so WITHOUT collectives a single step is issued eagerly
        # (200.9 against 207.9 us; run_many captures several steps per graph and replays at 199.9); WITH collectives the
        # eager step idles ~20 us inside itself (the event packets around each all-reduce) and the graph wins (207.8
        # against 220.0 us), so a multi-rank step is captured whenever the backend can be (RCCL).
        if use_graph is None:
            use_graph = self.collectives
        self.use_graph = bool(use_graph and dev.type == "cuda" and capturable)
        # the two keys live with the object: every step's select hands them back empty
        self._keys = [torch.full((batch,), KEY_EMPTY, dtype=torch.int64, device=dev) for _ in range(2)]
        self._R_fine = torch.empty((batch, self.seeds * self.D.shape[0], 3, 3), dtype=torch.float32, device=dev)
        self._klist = (torch.full((batch, self.seeds), KEY_EMPTY, dtype=torch.int64, device=dev)
                       if self.seeds > 1 or self.modes else None)
        if self.modes:   # everything the mode selection and the per-mode results write to lives with the object
            n1, K = self.R_coarse.shape[-3], self.modes
            self._block_keys = torch.full((batch, K), KEY_EMPTY, dtype=torch.int64, device=dev)
            self._block_off = (torch.arange(K, dtype=torch.int64, device=dev) * self.D.shape[0])[None]
            self._modes_ws = (ops.topk_modes_workspace(batch, n1, K, dev) if backend is None and dev.type == "cuda" else None)
            self._s_all = self._s_stage = None
            if self.collectives:
                self._s_all = torch.empty((batch, n1), dtype=torch.float32, device=dev)
                self._s_stage = torch.empty((self.world + 1, batch, -(-n1 // self.world)), dtype=torch.float32, device=dev)
        if self.resample:   # the draw list, the workspace and (multi-rank) the gathered row live with the object
            n1, M = self.R_coarse.shape[-3], self.D.shape[0]
            self._draws = torch.full((batch, M), -1, dtype=torch.int64, device=dev)
            self._resample_ws = (ops.resample_workspace(batch, n1, dev) if backend is None and dev.type == "cuda" else None)
            self._s_all = self._s_stage = None
            if self.collectives:
                self._s_all = torch.empty((batch, n1), dtype=torch.float32, device=dev)
                self._s_stage = torch.empty((self.world + 1, batch, -(-n1 // self.world)), dtype=torch.float32, device=dev)
        self._graph = None
        self._static = None
        can_fuse = backend is None and not self.collectives and self.world == 1 and dev.type == "cuda"
        if fused and not can_fuse:
            raise RuntimeError("the one-launch step needs one rank, no collectives and the HIP backend")
        self.fused = bool(fused)
        self._fused_state = ops.CoarseToFineState(batch, dev) if self.fused else None
        self._fused_out = {}     # slot -> the one-launch step's output buffers (a slot = one step of a multi-step graph)
        self._many = None        # (K, static inputs, captured graph, outputs) of run_many

    def _merge(self, key):
        if self.collectives:  # world > 1, or forced on a 1-rank group: same call, same captured node
            dist.all_reduce(key, op=dist.ReduceOp.MAX, group=self.group)
        return key

    @property
    def buffers(self):
        """The static input volumes ``(vol_src, vol_tgt)`` of the captured step (allocated on first use).  A producer that
        writes its volumes straight into them -- ``forward_2d3d(..., out=c2f.buffers)`` -- and then calls ``c2f()`` with no
        arguments replays the graph with no staging copy."""
        if self._static is None:
            dev = self.R_coarse.device
            self._static = tuple(torch.zeros((self.B, 16, 8, 8, 8), dtype=torch.float32, device=dev) for _ in range(2))
        return self._static

    # ---- the step, written once; runs eagerly or under capture
    def _step(self, vol_src, vol_tgt, slot: int = 0):
        o = self.ops
        if self.fused:
            r = o.coarse_to_fine(vol_src, vol_tgt, self.R_coarse, self.D, self.W1, self.W2, self.b2, state=self._fused_state,
                                 want_scores=self.want_scores, no_teams=self.no_teams, out=self._fused_out.setdefault(slot, {}))
            # (the refinement set is never materialised here: R_fine stays None)
            self.last = {"coarse_scores": r.get("coarse_scores"), "fine_scores": r.get("fine_scores"), "R_fine": None}
            return r["fine_score"], r["fine_idx"], r["R_pred"], r["coarse_score"], r["coarse_idx"]
        if self.modes:
            return self._step_modes(vol_src, vol_tgt, slot)
        if self.resample:
            return self._step_resample(vol_src, vol_tgt, slot)
        if self.seeds > 1:
            return self._step_seeds(vol_src, vol_tgt, slot)
        key1, key2 = self._keys
        kw = {"no_teams": True} if self.no_teams else {}
        Rc = self.R_coarse[self.c_lo:self.c_hi]
        s1, _, f_tgt = o.verify_pair(vol_src, vol_tgt, Rc, self.W1, self.W2, self.b2, n_offset=self.c_lo,
                                     want_scores=self.want_scores, best_key=key1, reset_best=False, want_feat_tgt=True, **kw)
        self._merge(key1)
        # Every rank holds the whole coarse set AND the whole refinement set D, so after the key all-reduce each
        # rank composes ALL N2 refinements of the winner locally (N2 * B threads) and scores its own slice of them.
        # After the second key all-reduce every rank knows both winning indices and already holds the winning
        # row: R_pred is a local gather -- two collectives per step, not three.
        R_fine_all = o.compose_rotations(key1, self.R_coarse, self.D, out=self._R_fine)
        R_fine = R_fine_all if self.world == 1 else R_fine_all[:, self.f_lo:self.f_hi]
        s2, _ = o.score_hypotheses(vol_src, f_tgt, R_fine, self.W1, self.W2, self.b2, n_offset=self.f_lo,
                                   want_scores=self.want_scores, best_key=key2, reset_best=False, **kw)
        self._merge(key2)
        score, idx, R_pred = o.select_rotation(key2, R_fine_all, n_offset=0, reset_key=True)
        coarse_score, coarse_idx, _ = o.select_rotation(key1, self.R_coarse, n_offset=0, reset_key=True)
        # this rank's slices of the two score sets and of the refinement set (None unless want_scores)
        self.last = {"coarse_scores": s1, "fine_scores": s2, "R_fine": R_fine if self.want_scores else None}
        score, R_pred = self._polish(vol_src, f_tgt, score, R_pred, slot)
        return score, idx, R_pred, coarse_score, coarse_idx

    def _polish(self, vol_src, f_tgt, score, R_pred, slot: int = 0):
        """The fine winner after ``polish_iters`` ascent steps (every rank on its own: same inputs, same bits)."""
        if self.polish_iters == 0:
            return score, R_pred
        R, s, theta = self.ops.polish_rotations(vol_src, f_tgt, R_pred[:, None], self.W1, self.W2, self.b2,
                                                iters=self.polish_iters, init_angle_deg=self.polish_angle_deg,
                                                ladder=self.polish_ladder, out=self._polish_out.setdefault(slot, {}))
        self.last["polish"] = {"score_before": score, "R_before": R_pred, "score_after": s[:, 0], "R_after": R[:, 0],
                               "theta": theta[:, 0]}
        return s[:, 0], R[:, 0]

    def _step_seeds(self, vol_src, vol_tgt, slot: int = 0):
        """The step with ``seeds = K > 1``: stage 2 scores the K*N2 refinements of the K best coarse hypotheses."""
        o = self.ops
        key2 = self._keys[1]
        kw = {"no_teams": True} if self.no_teams else {}
        Rc = self.R_coarse[self.c_lo:self.c_hi]
        # the coarse scores are kept: the K-list is selected from them (the scorer's own arg-max key is its first entry)
        s1, _, f_tgt = o.verify_pair(vol_src, vol_tgt, Rc, self.W1, self.W2, self.b2, n_offset=self.c_lo, want_scores=True,
                                     want_feat_tgt=True, **kw)
        klist = o.topk(s1, self.seeds, n_offset=self.c_lo, keys=self._klist, reset=True)
        if self.collectives:  # 8*B*K bytes per rank, then the merge: the same list on every rank, however N1 was cut
            klist = all_gather_topk(klist, group=self.group, merge_fn=o.merge_topk, force=True)
        # every rank holds the whole coarse set and D: all K*N2 refinements are composed locally, a slice of them scored
        R_fine_all = o.compose_rotations_topk(klist, self.R_coarse, self.D, out=self._R_fine)
        R_fine = R_fine_all if self.world == 1 else R_fine_all[:, self.f_lo:self.f_hi]
        s2, _ = o.score_hypotheses(vol_src, f_tgt, R_fine, self.W1, self.W2, self.b2, n_offset=self.f_lo,
                                   want_scores=self.want_scores, best_key=key2, reset_best=False, **kw)
        self._merge(key2)
        score, idx, R_pred = o.select_rotation(key2, R_fine_all, n_offset=0, reset_key=True)
        top_scores, top_idx, _ = o.select_topk(klist, self.R_coarse, n_offset=0)
        self.last = {"coarse_scores": s1 if self.want_scores else None, "fine_scores": s2,
                     "R_fine": R_fine if self.want_scores else None, "coarse_topk": (top_scores, top_idx)}
        score, R_pred = self._polish(vol_src, f_tgt, score, R_pred, slot)
        return score, idx, R_pred, top_scores[:, 0], top_idx[:, 0]

    def _step_modes(self, vol_src, vol_tgt, slot: int = 0):
        """The step with ``modes = K``: ``_step_seeds`` with ``topk_modes`` over the whole coarse row in place of ``topk``."""
        o = self.ops
        K, N2, B = self.modes, self.D.shape[0], self.B
        kw = {"no_teams": True} if self.no_teams else {}
        Rc = self.R_coarse[self.c_lo:self.c_hi]
        s1, _, f_tgt = o.verify_pair(vol_src, vol_tgt, Rc, self.W1, self.W2, self.b2, n_offset=self.c_lo, want_scores=True,
                                     want_feat_tgt=True, **kw)
        s_all = s1
        if self.collectives:  # modes do not compose across shards: the whole row on every rank, then ONE selection
            s_all = all_gather_scores(s1, self.R_coarse.shape[-3], group=self.group, force=True, out=self._s_all,
                                      staging=self._s_stage)
        sym = {} if self.symmetry is None else {"symmetry": self.symmetry}   # (None: the call is the previous one)
        klist = o.topk_modes(s_all, self.R_coarse, K, self.mode_angle_deg, keys=self._klist, workspace=self._modes_ws, **sym)
        R_fine_all = o.compose_rotations_topk(klist, self.R_coarse, self.D, out=self._R_fine)
        R_fine = R_fine_all if self.world == 1 else R_fine_all[:, self.f_lo:self.f_hi]
        s2, _ = o.score_hypotheses(vol_src, f_tgt, R_fine, self.W1, self.W2, self.b2, n_offset=self.f_lo, want_scores=True, **kw)
        # each mode's best refinement: the arg-max key of every N2-block (index inside the block) that this rank scored
        bk = self._block_keys
        if self.world == 1:
            bk.copy_(o.argmax(s2.view(B * K, N2), return_key=True).view(B, K))
        else:
            bk.fill_(KEY_EMPTY)
            for k in range(self.f_lo // N2, (self.f_hi - 1) // N2 + 1 if self.f_hi > self.f_lo else 0):
                a, b = max(self.f_lo, k * N2), min(self.f_hi, (k + 1) * N2)
                bk[:, k] = o.argmax(s2[:, a - self.f_lo:b - self.f_lo].contiguous(), n_offset=a - k * N2, return_key=True)
        self._merge(bk)   # the second collective, (B,K) keys wide
        bk = torch.where(klist == KEY_EMPTY, klist, bk)   # an EMPTY mode's block was composed around row 0: no result
        m_score, m_idx, m_R = o.select_rotation(bk.view(B * K), R_fine_all.view(B * K, N2, 3, 3), n_offset=0)
        m_score, m_idx, m_R = m_score.view(B, K), m_idx.view(B, K), m_R.view(B, K, 3, 3)
        # the fine winner: the same keys with the index moved to mode * N2 + idx (the index word counts down: no borrow)
        key2 = torch.where(bk == KEY_EMPTY, bk, bk - self._block_off).max(dim=1).values
        score, idx, R_pred = o.select_rotation(key2, R_fine_all, n_offset=0)
        top_scores, top_idx, _ = o.select_topk(klist, self.R_coarse, n_offset=0)
        self.last = {"coarse_scores": s_all if self.want_scores else None, "fine_scores": s2,
                     "R_fine": R_fine if self.want_scores else None, "coarse_topk": (top_scores, top_idx),
                     "modes": (m_score, m_idx, m_R)}
        if self.polish_iters > 0:
            R, s, theta = o.polish_rotations(vol_src, f_tgt, m_R, self.W1, self.W2, self.b2, iters=self.polish_iters,
                                             init_angle_deg=self.polish_angle_deg, ladder=self.polish_ladder,
                                             out=self._polish_out.setdefault(slot, {}))
            s = torch.where(bk == KEY_EMPTY, m_score, s)   # an EMPTY mode (a zero matrix went in) stays at -inf
            self.last["polish"] = {"score_before": m_score, "R_before": m_R, "score_after": s, "R_after": R, "theta": theta}
            score, best = s.max(dim=1)
            R_pred = R[torch.arange(B, device=R.device), best]
            idx = best * N2 + m_idx[torch.arange(B, device=R.device), best]
        return score, idx, R_pred, top_scores[:, 0], top_idx[:, 0]

    def _step_resample(self, vol_src, vol_tgt, slot: int = 0):
        """The step with ``resample=True``: stage 2 scores M draws from the coarse posterior, draw j refined by ``D[j]``."""
        o = self.ops
        key1, key2 = self._keys
        kw = {"no_teams": True} if self.no_teams else {}
        Rc = self.R_coarse[self.c_lo:self.c_hi]
        if self.collectives:  # a prefix needs the whole row: gather it, then every rank draws the same list
            s1, _, f_tgt = o.verify_pair(vol_src, vol_tgt, Rc, self.W1, self.W2, self.b2, n_offset=self.c_lo, want_scores=True,
                                         want_feat_tgt=True, **kw)
            s_all = all_gather_scores(s1, self.R_coarse.shape[-3], group=self.group, force=True, out=self._s_all,
                                      staging=self._s_stage)
            key1 = o.argmax(s_all, return_key=True)   # the coarse arg-max from the gathered row, locally: no key all-reduce
            coarse_score, coarse_idx, _ = o.select_rotation(key1, self.R_coarse, n_offset=0)
        else:
            s_all, _, f_tgt = o.verify_pair(vol_src, vol_tgt, Rc, self.W1, self.W2, self.b2, n_offset=0, want_scores=True,
                                            best_key=key1, reset_best=False, want_feat_tgt=True, **kw)
            coarse_score, coarse_idx, _ = o.select_rotation(key1, self.R_coarse, n_offset=0, reset_key=True)
        draws = o.resample(s_all, self.D.shape[0], self.resample_temperature, u=self.resample_u, out=self._draws,
                           workspace=self._resample_ws)
        draws[:, 0].copy_(coarse_idx)   # glue: D[0] = I, so the coarse winner itself is among the fine hypotheses
        R_fine_all = o.compose_rotations_indexed(draws, self.R_coarse, self.D, out=self._R_fine)
        R_fine = R_fine_all if self.world == 1 else R_fine_all[:, self.f_lo:self.f_hi]
        s2, _ = o.score_hypotheses(vol_src, f_tgt, R_fine, self.W1, self.W2, self.b2, n_offset=self.f_lo,
                                   want_scores=self.want_scores, best_key=key2, reset_best=False, **kw)
        self._merge(key2)
        score, idx, R_pred = o.select_rotation(key2, R_fine_all, n_offset=0, reset_key=True)
        self.last = {"coarse_scores": s_all if self.want_scores else None, "fine_scores": s2,
                     "R_fine": R_fine if self.want_scores else None, "resample": draws}
        score, R_pred = self._polish(vol_src, f_tgt, score, R_pred, slot)
        return score, idx, R_pred, coarse_score, coarse_idx

    def check(self):
        """Host sync.  Raises if a one-launch step abandoned its device-wide meeting point (another kernel held compute units
        for about a second: the stage-1 scores were then taken against an incomplete coarse winner).  The kernel poisons such a
        step's outputs (NaN scores, index -1, NaN rotation), so the failure cannot be mistaken for a result; this names it."""
        if self.fused and self._fused_state.gave_up():
            raise RuntimeError("ahv_coarse_to_fine_f32: a workgroup gave up the meeting point (the device was shared with "
                               "another kernel for ~1 s); the outputs of that step AND of every step since are poisoned "
                               "(NaN / -1): the error word is sticky. Call clear_error() to use this object again, or use "
                               "fused=False when other work runs on the GPU.")

    def clear_error(self):
        """After a give-up (``check()`` raised): reset the one-launch step's state -- keys, meeting-point counters, the sticky
        error word -- so that the next step runs clean."""
        if self._fused_state is not None:
            self._fused_state.clear_error()

    def _reset_keys(self):
        """After an exception inside a step the persistent keys may hold half a step's winners: hand them back empty."""
        for k in self._keys:
            k.fill_(KEY_EMPTY)
        if self._fused_state is not None:
            self._fused_state.keys.fill_(KEY_EMPTY)
            self._fused_state.sync[:-1].zero_()

    @torch.no_grad()
    def __call__(self, vol_src: Optional[torch.Tensor] = None, vol_tgt: Optional[torch.Tensor] = None):
        """vol_src, vol_tgt (B,16,8,8,8) -> (fine score (B,), fine index (B,), R_pred (B,3,3),
        coarse score (B,), coarse index (B,)).  With ``use_graph`` the outputs are static buffers that
        the next call overwrites; called with no arguments the step runs on ``self.buffers`` as they are."""
        if (vol_src is None) != (vol_tgt is None):
            raise RuntimeError("pass both volumes or neither")
        if not self.use_graph:
            if vol_src is None:
                vol_src, vol_tgt = self.buffers
            try:
                return self._step(vol_src, vol_tgt)
            except Exception:
                self._reset_keys()  # a step that raised midway must not leave its winners to the next one
                raise
        static = self.buffers
        if vol_src is not None and vol_src.data_ptr() != static[0].data_ptr():
            static[0].copy_(vol_src)
        if vol_tgt is not None and vol_tgt.data_ptr() != static[1].data_ptr():
            static[1].copy_(vol_tgt)
        if self._graph is None:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):  # warm-up outside capture (lazy initialisation inside the launchers / RCCL)
                for _ in range(2):
                    self._step(*static)
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                self._out = self._step(*static)
        self._graph.replay()
        return self._out

    @torch.no_grad()
    def run_many(self, vol_src: Optional[torch.Tensor] = None, vol_tgt: Optional[torch.Tensor] = None, steps: int = 8):
        """``steps`` consecutive verify steps -- volumes ``(steps, B, 16, 8, 8, 8)`` -- as ONE hipGraph launch; returns a list
        of ``steps`` result tuples (static buffers with ``use_graph``).  Why it exists: a hipGraphLaunch leaves the device
        idle for ~9 us between the last kernel of one replay and the first of the next (ROCm 7.2, `rocprofv3
        --kernel-trace`, profiles/r06_graph_timeline.txt) while plain launches follow each other with no gap, so a graph of
        ONE 0.2-ms step replays 4 % slower than the same step issued eagerly; with several steps per graph the gap is paid
        once per replay and the captured steps run back to back.  Without ``use_graph`` the steps are issued eagerly.
        Called with no volumes it runs on the static inputs as they are (``many_buffers(steps)``)."""
        if (vol_src is None) != (vol_tgt is None):
            raise RuntimeError("pass both volumes or neither")
        if not self.use_graph:
            if vol_src is None:
                vol_src, vol_tgt = self.many_buffers(steps)
            try:
                return [self._step(vol_src[k], vol_tgt[k], slot=k) for k in range(steps)]
            except Exception:
                self._reset_keys()
                raise
        static = self.many_buffers(steps)
        if vol_src is not None and vol_src.data_ptr() != static[0].data_ptr():
            static[0].copy_(vol_src)
            static[1].copy_(vol_tgt)
        if self._many[2] is None:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):  # warm-up outside capture
                for k in range(steps if self.polish_iters > 0 else min(2, steps)):   # (polishing builds a slot's buffers on first use)
                    self._step(static[0][k], static[1][k], slot=k)
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                outs = [self._step(static[0][k], static[1][k], slot=k) for k in range(steps)]
            self._many[2], self._many[3] = graph, outs
        self._many[2].replay()
        return self._many[3]

    def many_buffers(self, steps: int):
        """Static inputs ``(vol_src, vol_tgt)``, each ``(steps, B, 16, 8, 8, 8)``, of ``run_many``."""
        if self._many is None or self._many[0] != steps:
            dev = self.R_coarse.device
            bufs = tuple(torch.zeros((steps, self.B, 16, 8, 8, 8), dtype=torch.float32, device=dev) for _ in range(2))
            self._many = [steps, bufs, None, None]
        return self._many[1]
