"""Joint pose inference over an unposed image set: all the rotations of V images at once, on the device.

Build-defined: the reference's CO3D loader and ``get_permutations(eval_time=True)`` produce every ordered pair of a sequence's
frames, and the reference scores each pair on its own.  V (V - 1) independent arg-maxes do not agree with each other around a
cycle, and one bad pair -- more than 90 degrees apart, outside the range the network is trained for -- is simply wrong.
``PoseGraph`` is the standard remedy (RelPose's joint inference): absolute rotations ``A_v`` with ``A_root = I`` such that every
edge ``i -> j`` sees ``A_j A_i^T``.

1. pairwise   ``verify_pair`` over the B*E (source, target) samples against the shared hypotheses ``R0`` and
              ``select_rotation``: per edge its best rotation ``pair_R`` and score ``pair_score``
2. tree       ``pose_graph_init``: a maximum spanning tree of the most confident pairs from the root, and the rotations it implies
3. ascent     ``sweeps`` Gauss-Seidel sweeps over the nodes in index order, the root skipped.  Per node k: ``pose_graph_propose``
              (the current rotation, what each neighbour implies, noise of sweep s's scale around the current rotation, fresh
              Haar slots) -> ``pose_graph_score`` (the scorer over the node's D_k incident edges and the mean over them) ->
              ``pose_graph_commit`` (the arg-max becomes ``A_k``)

Slot 0 of every update is the node's current rotation bit for bit and a score is a function of (volumes, weights, R) alone, so
the mean score of a node's edges never decreases.  The incident edges' volumes are staged once per solve (``gather_views``),
outside the sweeps; everything between the pairwise stage and the result is device memory the object owns, and the solution is
a function of (seed, solve counter, inputs).

Not built: per-edge weights decided on the device (from ``pair_score`` or the posterior's mode mass), symmetric objects, more
than one candidate solution per node, the compact / angle-limited fusion, and more than one rank (a graph is a few dozen
samples of a few hundred candidates: there is nothing to shard)."""
from __future__ import annotations

import collections

import torch

from . import ops
from .dist import KEY_EMPTY

PoseGraphResult = collections.namedtuple("PoseGraphResult", ["A", "node_score", "pair_R", "pair_score", "parent_edge", "reached",
                                                             "init_A"])

_VOL = (16, 8, 8, 8)
_NEEDS = ("verify_pair", "select_rotation", "track_advance", "gather_views", "pose_graph_init", "pose_graph_propose",
          "pose_graph_score", "pose_graph_commit")


class PoseGraph:
    """``backend`` provides ``verify_pair, select_rotation, track_advance, gather_views, pose_graph_init, pose_graph_propose,
    pose_graph_score, pose_graph_commit`` with the signatures of ``3dahv_amd.ops`` -- the default and the only product backend:
    HIP kernels, no CPU path; CPU tests inject an oracle-backed object to execute the control flow.

    ``n_views=V`` images and ``edges``, a list of directed ``(i, j)`` (None: every ordered pair); a node's degree counts both
    directions and must not exceed ``AHV_VIEWS_MAX`` = 16, so the complete ordered graph goes up to V = 9.  ``candidates=N`` per
    node update, of which the last ``n_fresh`` are Haar rotations; N >= 1 + D_k + n_fresh for every node.  Sweep s uses
    ``sigma_deg[min(s, len - 1)]``.  ``edge_weights``: E host floats >= 0 (None: ones), 0 removes an edge from every update (not
    from the tree, which goes by ``pair_score``); a node whose edges all weigh 0 is refused.

    ``solve(vol_src (B,E,16,8,8,8), vol_tgt (B,E,16,8,8,8), R0 (N0,3,3))`` -- the encoder's volumes of every edge's ordered pair
    -- returns ``PoseGraphResult(A (B,V,3,3), node_score (B,V), pair_R (B,E,3,3), pair_score (B,E), parent_edge (B,V), reached
    (B,V), init_A (B,V,3,3))``: the joint solution and the mean score of each node's edges at its last update (NaN for the root
    and a node without an edge), the independent arg-maxes it started from, the tree and the tree's solution.  The tensors are
    the object's own buffers, valid until the next ``solve``.  ``relative()`` gives ``A_j A_i^T`` per edge.

    Every solve starts by moving the solve counter on the device (``track_advance``), so two solves of one object draw
    different noise and two objects with one seed the same.  After construction a solve allocates nothing but what the
    pairwise stage's ``R0`` needs.

    ``use_graph=True`` (HIP backend only; refused with a ``backend`` or on the CPU): everything after the pairwise stage -- the
    counter, the tree, the staging and all sweeps -- is captured into one hipGraph by the first solve and replayed by every
    later one.  The capturing solve synchronises with the host (a capture starts from an idle device)."""

    def __init__(self, W1: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor, n_views: int, edges=None, batch: int = 1,
                 candidates: int = 128, sweeps: int = 8, sigma_deg=(6, 4, 3, 2, 1.5, 1, 0.75, 0.5), n_fresh: int = 0,
                 root: int = 0, seed: int = 0, edge_weights=None, use_graph: bool = False, backend=None):
        dev = W1.device
        self.ops = ops if backend is None else backend
        missing = [n for n in _NEEDS if not hasattr(self.ops, n)]
        if missing:
            raise RuntimeError("PoseGraph needs a backend that provides %s" % ", ".join(missing))
        hip = backend is None and dev.type == "cuda"
        if use_graph and not hip:
            raise RuntimeError("use_graph=True needs the HIP backend on a GPU (backend=None, weights on the device)")
        self.use_graph = bool(use_graph)
        self.W1, self.W2, self.b2 = W1, W2, b2
        self.topology = top = ops.PoseGraphTopology(n_views, edges, root, device=dev)
        self.V, self.E, self.B = top.n_views, top.n_edges, int(batch)
        if not 1 <= self.B or self.B * self.E > 65535:
            raise RuntimeError("batch = %d: need 1 <= batch and batch * E = %d <= 65535 (the pairwise stage is one launch)"
                               % (self.B, self.B * self.E))
        self.N, self.n_fresh, self.sweeps = int(candidates), int(n_fresh), int(sweeps)
        if self.n_fresh < 0:
            raise RuntimeError("n_fresh = %d must be >= 0" % self.n_fresh)
        if not 0 <= self.sweeps <= 256:
            raise RuntimeError("sweeps = %d outside 0..256" % self.sweeps)
        for k, d in enumerate(top.degree):
            if self.N < 1 + d + self.n_fresh:
                raise RuntimeError("candidates = %d do not hold 1 + D_k + n_fresh = 1 + %d + %d slots of node %d"
                                   % (self.N, d, self.n_fresh, k))
        if self.N >= 1 << 31:
            raise RuntimeError("candidates = %d must be below 2^31" % self.N)
        self.sigma_deg = [float(s) for s in (sigma_deg if isinstance(sigma_deg, (list, tuple)) else [sigma_deg])]
        if not self.sigma_deg:
            raise RuntimeError("sigma_deg is empty")
        for s in self.sigma_deg:
            ops._angle_rad(s, "sigma_deg")                # raises unless finite and >= 0
        self.seed = int(seed)
        self.nodes = [k for k in range(self.V) if k != top.root and top.degree[k] > 0]   # the visiting order of a sweep
        self.weights = None
        if edge_weights is not None:
            w = [float(x) for x in (edge_weights.tolist() if isinstance(edge_weights, torch.Tensor) else edge_weights)]
            if len(w) != self.E:
                raise RuntimeError("edge_weights must hold E = %d values, got %d" % (self.E, len(w)))
            if not all(x >= 0.0 and x < float("inf") for x in w):
                raise RuntimeError("edge_weights must be finite and >= 0")
            self.weights = {k: [w[e] for e, _ in top.incident[k]] for k in self.nodes}
            for k, wk in self.weights.items():
                if not any(x > 0.0 for x in wk):
                    raise RuntimeError("edge_weights leave node %d without an edge (all its weights are 0)" % k)
        B, V, E, N = self.B, self.V, self.E, self.N
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        self._pair_key = torch.full((B * E,), KEY_EMPTY, dtype=torch.int64, device=dev)
        self._pair = (f(B * E), torch.empty((B * E,), dtype=torch.int64, device=dev), f(B * E, 3, 3))   # select_rotation's out
        self._A, self._init_A, self._node_score = f(B, V, 3, 3), f(B, V, 3, 3), f(B, V)
        self._tree = (i32(B, V), i32(B, V))
        self._Q, self._fused = f(B, N, 3, 3), f(B, N)
        self._key = torch.full((B,), KEY_EMPTY, dtype=torch.int64, device=dev)
        self._counter = torch.zeros((1,), dtype=torch.int64, device=dev)
        self._u = f(B)
        # per node: the staged volumes of its incident edges, its Rrel, its workspace and the staging plan
        self._staged = {k: (f(B, top.degree[k], *_VOL), f(B, top.degree[k], *_VOL)) for k in self.nodes}
        self._Rrel = {k: f(B, top.degree[k], N, 3, 3) for k in self.nodes}
        self._ws = {k: ops.pose_graph_workspace(B, top.degree[k], N, dev) if hip else None for k in self.nodes}
        self._plan = {k: self._staging_plan(k, dev) for k in self.nodes}
        self._static = None
        self._graph = None
        self._result = None
        self._vols = None     # the volumes of the last solve (use_graph: the static buffers)

    def _staging_plan(self, k, dev):
        """``gather_views`` takes at most ``AHV_VIEWS_MAX`` source rows per sample.  E <= 16: one call per node and tensor with
        the node's edge ids for every sample.  Else the edge axis is cut into windows of 16 edges and, a window's rows being
        adjacent in memory only within one sample, each (sample, window that holds an incident edge) is a call of its own: a
        list of ``(b, first edge, edges in the window, first staged row, idx (1,K) int32)``."""
        ids = [e for e, _ in self.topology.incident[k]]
        vmax = ops._lib.AHV_VIEWS_MAX
        if self.E <= vmax:
            return [(None, 0, self.E, 0, torch.tensor([ids] * self.B, dtype=torch.int32, device=dev))]
        plan = []
        for w0 in range(0, self.E, vmax):
            rows = [(d, e - w0) for d, e in enumerate(ids) if w0 <= e < w0 + vmax]   # ids ascend: the rows are adjacent
            if rows:
                idx = torch.tensor([[r for _, r in rows]], dtype=torch.int32, device=dev)
                plan += [(b, w0, min(vmax, self.E - w0), rows[0][0], idx) for b in range(self.B)]
        return plan

    @property
    def buffers(self):
        """The static input volumes ``(vol_src, vol_tgt)``, each ``(B,E,16,8,8,8)``, of the captured solve (allocated on first
        use): write the pairs' volumes there and call ``solve(None, None, R0)`` to solve with no staging copy."""
        if self._static is None:
            self._static = tuple(torch.zeros((self.B, self.E) + _VOL, dtype=torch.float32, device=self.W1.device) for _ in range(2))
        return self._static

    @property
    def counter(self) -> torch.Tensor:
        """The solve counter, one int64 on the device: a solve moves it by one and draws its noise from the new value."""
        return self._counter

    def _stage(self, vs, vt):
        for k in self.nodes:
            for src, dst in ((vs, self._staged[k][0]), (vt, self._staged[k][1])):
                for b, w0, width, d0, idx in self._plan[k]:
                    if b is None:
                        self.ops.gather_views(src, idx, out=dst)
                    else:
                        self.ops.gather_views(src[b:b + 1, w0:w0 + width], idx, out=dst[b:b + 1, d0:d0 + idx.shape[1]])

    def _ascent(self, vs, vt):
        o, top = self.ops, self.topology
        pair_score, _, pair_R = self._pair
        pair_R, pair_score = pair_R.view(self.B, self.E, 3, 3), pair_score.view(self.B, self.E)
        o.track_advance(self._counter, self.seed, self.B, u=self._u)
        o.pose_graph_init(pair_R, pair_score, top, out=(self._A,) + self._tree)
        self._init_A.copy_(self._A)
        self._node_score.fill_(float("nan"))
        self._stage(vs, vt)
        for s in range(self.sweeps):
            sigma = self.sigma_deg[min(s, len(self.sigma_deg) - 1)]
            for k in self.nodes:
                Q, Rrel = o.pose_graph_propose(self._A, pair_R, pair_score, top, k, self.N, sigma, sweep=s, seed=self.seed,
                                               counter=self._counter, n_fresh=self.n_fresh, out=(self._Q, self._Rrel[k]))
                o.pose_graph_score(self._staged[k][0], self._staged[k][1], Rrel, self.W1, self.W2, self.b2,
                                   weights=None if self.weights is None else self.weights[k], workspace=self._ws[k],
                                   scores_out=self._fused, best_key=self._key)
                o.pose_graph_commit(self._key, Q, self._A, self._node_score, k)

    @torch.no_grad()
    def solve(self, vol_src, vol_tgt, R0: torch.Tensor) -> PoseGraphResult:
        B, E = self.B, self.E
        if (vol_src is None) != (vol_tgt is None):
            raise RuntimeError("give both volumes, or neither (the static buffers are then solved as they are)")
        if vol_src is None:
            vs, vt = self.buffers
        else:
            for name, v in (("vol_src", vol_src), ("vol_tgt", vol_tgt)):
                if tuple(v.shape) != (B, E) + _VOL:
                    raise RuntimeError("%s must be (B,E,16,8,8,8) = %s, got %s" % (name, (B, E) + _VOL, tuple(v.shape)))
            vs, vt = vol_src.detach().contiguous(), vol_tgt.detach().contiguous()
            if self.use_graph:
                for dst, src in zip(self.buffers, (vs, vt)):
                    dst.copy_(src)
                vs, vt = self.buffers
        if R0.dim() != 3 or tuple(R0.shape[1:]) != (3, 3) or R0.shape[0] < 1:
            raise RuntimeError("R0 must be (N0,3,3), the hypotheses every pair is scored against, got %s" % (tuple(R0.shape),))
        self.ops.verify_pair(vs.view((B * E,) + _VOL), vt.view((B * E,) + _VOL), R0, self.W1, self.W2, self.b2, want_scores=False,
                             best_key=self._pair_key, reset_best=True)
        self.ops.select_rotation(self._pair_key, R0, out=self._pair)
        self._vols = (vs, vt)
        return self.ascend()

    @torch.no_grad()
    def ascend(self) -> PoseGraphResult:
        """Everything after the pairwise stage once more, on the last ``solve``'s pairwise estimates and volumes: the counter
        moves, so the noise is new.  What ``solve`` ends with, and what a captured solve replays."""
        if self._vols is None:
            raise RuntimeError("ascend(): no solve yet")
        B, E = self.B, self.E
        if not self.use_graph:
            self._ascent(*self._vols)
        else:
            if self._graph is None:
                torch.cuda.synchronize()
                self._graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self._graph):
                    self._ascent(*self._vols)
            self._graph.replay()
        score, _, R = self._pair
        self._result = PoseGraphResult(self._A, self._node_score, R.view(B, E, 3, 3), score.view(B, E), self._tree[0],
                                       self._tree[1], self._init_A)
        return self._result

    def relative(self, A: torch.Tensor | None = None) -> torch.Tensor:
        """``A_j A_i^T`` per edge ``(B,E,3,3)`` of the last solution (or of ``A (B,V,3,3)``)."""
        if A is None:
            if self._result is None:
                raise RuntimeError("relative(): no solve yet")
            A = self._result.A
        i = torch.tensor([e[0] for e in self.topology.edges], device=A.device)
        j = torch.tensor([e[1] for e in self.topology.edges], device=A.device)
        return A[:, j] @ A[:, i].transpose(-1, -2)
