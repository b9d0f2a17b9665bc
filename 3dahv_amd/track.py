"""Pose tracking over a frame sequence: a particle filter on SO(3) whose step stays on the device.

Build-defined: the reference scores every image pair from scratch against 50 000 random rotations (test_co3d.py:106,137-146).
A video is frame after frame of one object, so the pose posterior of one frame is the prior of the next.  ``PoseTracker`` keeps
M pose particles per sample.  Per frame it

1. ``track_advance``       moves the device step counter and draws the resampling offsets ``u``,
2. ``resample``            draws M particles in proportion to the previous frame's posterior (systematic draws),
3. ``diffuse_rotations``   moves each by a small random rotation (fresh noise generated on the device from the counter), keeps
                           the previous arg-max untouched in slot 0 (the elite) and fills the last ``n_fresh`` slots with new
                           Haar rotations (re-acquisition after a lost track); with ``motion="constant_velocity"`` the step is
                           ``predict_rotations`` instead: every particle carries a velocity (a body-frame rotation vector per
                           frame) that is resampled with it, perturbed and applied before the noise, and slot 1 is the previous
                           arg-max moved by its own velocity (``coast``),
4. ``verify_pair``         scores the set against the new frame (the fused scorer, scores kept),
5. ``select_rotation``     reports the MAP pose,

and with ``posterior=True`` ``pose_posterior`` with the MAP pose as the single anchor: the mass within ``mode_angle_deg`` of it,
the mean pose, the spread and the entropy.  Everything between two frames is device memory the tracker owns; the trajectory is a
function of (seed, inputs) alone.

One rank: a particle set is a few hundred to a few thousand rotations, there is nothing to shard.  With an initialised process
group every rank runs the same tracker on the same inputs and computes the same bytes; no collective is issued.
The random walk (``motion="walk"``, the default) holds a pose that moves about sigma per frame; a pose that moves steadily
faster needs ``motion="constant_velocity"``: the particles whose velocity matches the motion are the ones that score, so the
filter learns the velocity from the scores alone.
Per frame the tracker reports the arg-max of that frame's own scores, which is wrong on a frame that is not a good view of
the object (occluded, blurred, a cut to something else).  ``history=H`` keeps the particle sets and scores of the last H frames
in a ring and runs one Viterbi step per frame over it (``smooth_step``, after ``verify_pair``): MAP sequence estimation over
the particle history (Godsill, Doucet and West 2001).  ``smoothed()`` backtraces the most probable trajectory; a frame whose
scores disagree with its neighbours is bridged by the motion prior, or left by paying ``smooth_jump``.  Smoothing observes and
never steers: every ``TrackStep`` is the same bytes with and without it.
The Viterbi path is one pose per past frame and says nothing about how sure it is.  ``marginals=True`` (with ``history``) also
runs the forward recursion of the same model per frame (``marginal_step``, after ``smooth_step``), and
``smoothed_marginals()`` the backward one: a row of log-weights per past frame, the probability that the trajectory passes
through each particle given every recorded frame, which ``pose_posterior`` turns into a smoothed mean pose, its spread, the
mass that agrees with the frame's most probable particle and the entropy.
A symmetric object has |G| equivalent clusters of particles, and the MAP pose hops between them from frame to frame.
``symmetry=`` (a ``rotations.Symmetry`` in the source view's frame) folds the predicted set into the fundamental domain around the
previous frame's MAP pose (``sym_fold``, one launch before ``verify_pair``): the cloud lives in one domain, so the MAP pose, the
posterior and both smoothers need no change.
One reference view cannot carry a pose through a full turn: the network is trained on pairs closer than ``DATA.VIEW_THR`` (90
degrees, the limit ``fuse_view_scores`` cites), so past that range a single-reference tracker has no trustworthy score.
``views=A`` gives the tracker V posed reference views: its particles are then ABSOLUTE poses Q in the frame of ``A`` (view v sees
``Q A_v^T``), and per step it picks, on the device, the ``views_per_step`` views nearest the previous MAP pose
(``nearest_views``), stages their volumes (``gather_views``) and scores the set against those alone, fused under the angle
limit (``verify_views_staged``) -- all inside the captured chain, with no host read.
A constant ``sigma_deg`` is wrong for a pose whose speed changes: too narrow and the cloud is left behind, too wide and every
slow frame pays for it, and after an abrupt change of pose a fixed tracker may never find the object again.  ``adapt=
AdaptiveNoise(...)`` lets the device decide: one launch after ``select_rotation`` (``track_control``) measures the innovation --
how far the MAP pose landed from where the previous one predicted it -- and the MAP score, and writes the next frame's sigma,
sigma_vel and n_fresh into a control record the predict step (``predict_rotations_controlled``) reads.  Not the entropy: this
filter resamples every step, so the weights of a converged cloud are as flat as those of a lost one.
Not built: adaptation together with views or symmetry and of the smoothers' transition scale, per-view weights other than present / absent and per-particle view selection inside
the tracker, the compact multi-view path inside the tracker, symmetry together with views, a fixed-lag marginal
inside the captured step, the velocity-noise term of the constant-velocity transition (the smoother's transition is
pose-only), and symmetry-aware transitions inside the smoothers (the fold makes them unnecessary for a tracked cloud).
"""
from __future__ import annotations

import collections
import math
from typing import Optional

import torch

from . import ops
from .dist import KEY_EMPTY

TrackStep = collections.namedtuple(
    "TrackStep", ["score", "idx", "R_map", "particles", "scores", "draws", "R_mean", "spread_deg", "mode_mass", "entropy",
                  "reacquired"])


class AdaptiveNoise:
    """The rule ``PoseTracker(adapt=...)`` runs on the device per step (``ops.track_control``): the running per-axis variance of
    the motion ``m <- (1 - rate) m + rate a^2 / 3`` from the innovation ``a``, the next frame's ``sigma = clamp(gain sqrt(m),
    sigma_min_deg, sigma_max_deg)``, and below ``score_floor`` (None: never) a lost track: ``sigma_max_deg`` and
    ``n_fresh_lost`` fresh slots (None: the tracker's ``n_fresh``).  ``gain`` is above 1 because the innovation of a cloud that
    lags under-estimates the motion: at 1.0 the tracker loses an accelerating sequence that 1.5 holds."""

    def __init__(self, sigma_min_deg: float = 0.5, sigma_max_deg: float = 8.0, gain: float = 1.5, rate: float = 0.5,
                 score_floor: Optional[float] = None, n_fresh_lost: Optional[int] = None):
        self.sigma_min_deg, self.sigma_max_deg = float(sigma_min_deg), float(sigma_max_deg)
        if not 0.0 < ops._angle_rad(self.sigma_min_deg, "sigma_min_deg") <= ops._angle_rad(self.sigma_max_deg, "sigma_max_deg"):
            raise RuntimeError("sigma_min_deg = %r and sigma_max_deg = %r: need 0 < sigma_min <= sigma_max"
                               % (sigma_min_deg, sigma_max_deg))
        self.gain, self.rate = float(gain), float(rate)
        if not (self.gain > 0.0 and math.isfinite(self.gain)):
            raise RuntimeError("gain = %r must be finite and > 0" % (gain,))
        if not 0.0 < self.rate <= 1.0:
            raise RuntimeError("rate = %r outside (0, 1]" % (rate,))
        self.score_floor = None if score_floor is None else float(score_floor)
        if self.score_floor is not None and math.isnan(self.score_floor):
            raise RuntimeError("score_floor is NaN (None: no floor)")
        self.n_fresh_lost = None if n_fresh_lost is None else int(n_fresh_lost)
        if self.n_fresh_lost is not None and self.n_fresh_lost < 0:
            raise RuntimeError("n_fresh_lost = %d must be >= 0" % self.n_fresh_lost)


class PoseTracker:
    """``backend`` provides ``track_advance, resample, diffuse_rotations, verify_pair, select_rotation`` (and ``pose_posterior``
    with ``posterior=True``) with the signatures of ``3dahv_amd.ops`` -- the default and the only product backend: HIP kernels,
    no CPU path; CPU tests inject an oracle-backed object to execute the control flow.

    ``init(vol_src, vol_tgt, R_init)`` scores the hypotheses ``R_init (N0,3,3)`` / ``(B,N0,3,3)`` (eagerly); they, with their
    scores, are the particle set the first step draws from.  ``step(vol_src, vol_tgt)`` is the sequence of the module
    docstring: ``vol_src`` is the reference view's volume, ``vol_tgt`` the frame's.  Both return a ``TrackStep``: ``score (B,)``,
    ``idx (B,)`` (the winner's slot) and ``R_map (B,3,3)``; ``particles (B,M,3,3)``, ``scores (B,M)`` and ``draws (B,M)`` (the
    previous set's indices the slots were drawn from; None for ``init``); with ``posterior``: ``R_mean (B,3,3)``, ``spread_deg``,
    ``mode_mass`` and ``entropy`` (B,), else None; ``reacquired (B,)`` bool, true when the winner sits in a fresh slot.

    The tracker owns every buffer of a step, ping-pong: two particle sets, two score rows, two keys, two output sets, the draw
    list, the workspaces, ``u`` and the step counter.  A step reads one half and writes the other, so a ``TrackStep`` stays
    valid until the step after the next one.  After the first step a step allocates nothing (``posterior=True``: the
    ``pose_posterior`` outputs are that op's own).

    ``motion="constant_velocity"`` (``backend`` then also provides ``predict_rotations``): the tracker owns two more ping-pong
    buffers ``(B,M,3)``, the particles' velocities, ``.velocities`` after a step (valid as long as that step's particles).  The
    first step after ``init`` starts from zero velocities.  ``sigma_vel_deg`` is the scale of the velocity noise per frame,
    ``damping`` in [0, 1] multiplies the velocity each frame, ``max_speed_deg`` limits ``|v|`` (None: no limit) and ``coast``
    gives slot 1 to the previous arg-max moved by its own velocity with no noise; ``reacquired`` then starts behind that slot.
    Slot 0 carries the previous arg-max bit for bit and a score is a function of (volumes, weights, R) alone, so on an
    unchanged frame the reported score never decreases.

    ``history=H >= 2`` (``backend`` then also provides ``smooth_step`` and ``smooth_backtrace``): the tracker owns a ring of H
    frames (``ops.smooth_history``) and every step ends with ``smooth_step`` on the step's particles and scores -- with the
    constant-velocity model also its velocities and the damping, so that a transition is measured from the pose a particle
    predicts.  ``smooth_sigma_deg`` is the scale of the transition (None: ``sigma_deg``, and sqrt(sigma_deg^2 + sigma_vel_deg^2)
    with ``motion="constant_velocity"``), ``smooth_jump`` the price, in nats, of an arbitrary jump.  ``smoothed(frames)`` returns
    the ``SmoothedPath(idx (B,F), R (B,F,3,3))`` over the last ``min(frames, steps since init, H)`` frames, oldest first: the
    fixed-lag pose of frame t - L is ``path.R[:, -1 - L]``.  ``init`` restarts the counter, which hides every older slot; the
    set ``init`` scores is not recorded (the first frame of the path is the first ``step``).  ``history=0``: none of this, the
    calls of a step are the previous ones.

    ``marginals=True`` (needs ``history``; ``backend`` then also provides ``marginal_step`` and ``marginal_smooth``): the
    tracker owns an ``ops.marginal_history`` beside the ring and every step issues ``marginal_step`` right after
    ``smooth_step``, with the same scale and jump.  It observes and never steers: every ``TrackStep``, the ring and
    ``smoothed()`` are the same bytes with and without it.  ``smoothed_marginals()`` returns the marginals.

    ``symmetry=sym`` (``backend`` then also provides ``sym_fold``; refused at construction otherwise): every step issues one
    ``sym_fold`` after the predict step and before ``verify_pair``, in place on the step's particle buffer (and, with
    ``motion="constant_velocity"``, on its velocity buffer: a body-frame velocity turns with the element).  The single anchor is
    the previous frame's ``R_map``, with no angle limit; ``keep`` is 1, or 2 with ``coast``, so the elite (and the coasting slot)
    stay bit for bit.  The launch sits inside the captured chain.  The fresh Haar slots are folded too: they are still uniform on
    the quotient, but no longer the sampler's bytes.  ``symmetry=None``: the previous tracker, call for call.

    ``views=A`` (``(V,3,3)`` or ``(B,V,3,3)``, the reference views' absolute rotations; ``backend`` then also provides
    ``nearest_views``, ``gather_views`` and ``verify_views_staged``): particles, ``R_map``, the smoother's ring and the posterior are
    absolute poses in the frame of ``A``.  ``views_per_step=K`` views are scored per step (None: all V), ``max_view_angle_deg``
    is the angle limit of the fusion (None: none).  ``init(vol_refs (B,V,16,8,8,8), vol_query (B,16,8,8,8) or (B,V,16,8,8,8),
    R_init)`` scores ``R_init`` densely over all V views.  The tracker owns the selection (``view_selection``: ``idx (B,K)`` int32
    and ``A (B,K,3,3)``), the staged volumes ``buffers = (refs (B,K,16,8,8,8), query (B,K,16,8,8,8))`` and the workspace.
    ``select_views()`` is one launch whose anchor is the current MAP pose, read on the device; it returns the ``ViewSelection``
    the next step uses.  ``step(vol_refs (B,V,...), vol_query (B,...) or (B,V,...))`` runs select -> gather -> the chain;
    ``step(refs_K, query_K, staged=True)`` and ``step()`` run the chain on what is staged (the caller gathered the K references'
    inputs by ``view_selection.idx`` and encoded K pairs) and raise unless ``select_views()`` was called since the last step.
    The chain is that of the module docstring with ``verify_views_staged`` in the place of ``verify_pair``; the smoothers and the
    posterior follow unchanged: they see ``(Q, fused scores)``.  A particle no selected view sees within the angle limit scores
    -inf, and by ``resample``'s rule for such a score (it takes no part and is never drawn) it leaves no descendant; a fresh
    Haar slot far from the selected views therefore cannot re-acquire -- ``views_per_step=None`` scores every view and can.
    With ``use_graph=True`` each kind of step is captured once per half of the ping-pong -- selection, gather and the chain, or
    the chain alone for a staged step --, and the anchor being read on the device, a replay follows a selection that has
    changed since the capture; ``view_inputs`` are the static ``(B,V,...)`` inputs of the first kind, ``buffers`` of the second.
    ``symmetry=`` together with ``views`` is refused.  ``views=None``: the previous tracker, call for call.

    ``adapt=AdaptiveNoise(...)`` (``backend`` then also provides ``predict_rotations_controlled`` and ``track_control``; refused
    at construction otherwise, and together with ``views=`` or ``symmetry=``: not built): the tracker owns one control record
    ``(B,8)`` (``control_record``; ``control()`` decodes it on the host), which ``init`` resets to ``sigma_deg``,
    ``sigma_vel_deg`` and ``n_fresh``.  A step is ``track_advance`` -> ``resample`` -> ``predict_rotations_controlled`` (sigma,
    sigma_vel and n_fresh read from the record on the device; in the place of ``diffuse_rotations`` / ``predict_rotations``) ->
    ``verify_pair`` -> ``select_rotation`` -> ``track_control`` (in the place of the comparison that computes ``reacquired``; it
    writes the same buffer and the record of the next frame).  Posterior and smoothers follow unchanged; the ring's scale stays
    a constant, so with ``history`` ``smooth_sigma_deg`` must be given.  With ``use_graph=True`` all of it sits inside the
    captured chain and a replay follows the record.  ``adapt=None``: the previous tracker, call for call.

    ``use_graph=True`` (HIP backend only; refused with a ``backend`` or on the CPU): the first step after ``init`` reads the N0-sized set and runs eagerly; the two halves of
    the ping-pong are then captured as one hipGraph each, by the second and the third step, and every later step replays the
    graph of its half.  Each graph is the linear chain of the step's launches.  The two capturing steps synchronise with the
    host (a capture starts from an idle device); no other step does.  The step counter lives on the device and is
    moved there, so a replay draws new noise.  The static input volumes are ``.buffers``: write the frame's volumes there and
    call ``step()`` with no arguments to replay with no staging copy."""

    def __init__(self, W1: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor, particles: int, sigma_deg: float = 3.0,
                 n_fresh: int = 0, temperature: float = 0.02, max_angle_deg: Optional[float] = None, batch: int = 1,
                 seed: int = 0, posterior: bool = False, mode_angle_deg: float = 15.0, use_graph: bool = False, backend=None,
                 motion: str = "walk", sigma_vel_deg: float = 1.0, damping: float = 1.0, max_speed_deg: Optional[float] = None,
                 coast: bool = True, history: int = 0, smooth_sigma_deg: Optional[float] = None, smooth_jump: float = 8.0,
                 marginals: bool = False, symmetry=None, views: Optional[torch.Tensor] = None,
                 views_per_step: Optional[int] = None, max_view_angle_deg: Optional[float] = None,
                 adapt: Optional[AdaptiveNoise] = None):
        dev = W1.device
        self.ops = ops if backend is None else backend
        self.adapt = adapt
        if adapt is not None:
            if not isinstance(adapt, AdaptiveNoise):
                raise RuntimeError("adapt must be an AdaptiveNoise or None, got %s" % type(adapt).__name__)
            if views is not None or symmetry is not None:
                raise RuntimeError("adapt= together with views= or symmetry= is not built")
            if not all(hasattr(self.ops, n) for n in ("predict_rotations_controlled", "track_control")):
                raise RuntimeError("adapt= needs a backend that provides predict_rotations_controlled and track_control")
            if history and smooth_sigma_deg is None:
                raise RuntimeError("adapt= with history: give smooth_sigma_deg (the ring's scale stays a constant; it does not "
                                   "follow the adapted sigma)")
        self.symmetry = symmetry
        self.views = None
        if views is None:
            if views_per_step is not None or max_view_angle_deg is not None:
                raise RuntimeError("views_per_step and max_view_angle_deg belong to views=")
        else:
            if symmetry is not None:
                raise RuntimeError("symmetry= together with views= is not built")
            if not all(hasattr(self.ops, n) for n in ("nearest_views", "gather_views", "verify_views_staged")):
                raise RuntimeError("views= needs a backend that provides nearest_views, gather_views and verify_views_staged")
            if views.dim() not in (3, 4) or tuple(views.shape[-2:]) != (3, 3) or (views.dim() == 4 and views.shape[0] != int(batch)):
                raise RuntimeError("views must be (V,3,3) or (B,V,3,3) with B = %d, got %s" % (int(batch), tuple(views.shape)))
            self.V = int(views.shape[-3])
            if not 1 <= self.V <= ops._lib.AHV_VIEWS_MAX:
                raise RuntimeError("views: V = %d outside 1..%d" % (self.V, ops._lib.AHV_VIEWS_MAX))
            self.K = self.V if views_per_step is None else int(views_per_step)
            if not 1 <= self.K <= self.V:
                raise RuntimeError("views_per_step = %r outside 1..V = %d" % (views_per_step, self.V))
            self.max_view_angle_deg = None if max_view_angle_deg is None else float(max_view_angle_deg)
            if self.max_view_angle_deg is not None:
                ops.min_trace(self.max_view_angle_deg)    # raises outside (0, 180)
        if symmetry is not None and not hasattr(self.ops, "sym_fold"):
            raise RuntimeError("symmetry needs a backend that provides sym_fold")
        self.W1, self.W2, self.b2 = W1, W2, b2
        self.M, self.B = int(particles), int(batch)
        if not 1 <= self.M < (1 << 31):
            raise RuntimeError("particles = %d outside 1..2^31-1" % self.M)
        if not 1 <= self.B <= 65535:
            raise RuntimeError("batch = %d outside 1..65535" % self.B)
        self.n_fresh = int(n_fresh)
        if not 0 <= self.n_fresh <= self.M:
            raise RuntimeError("n_fresh = %d outside 0..particles = %d" % (self.n_fresh, self.M))
        self.sigma_deg = float(sigma_deg)
        self.max_angle_deg = None if max_angle_deg is None else float(max_angle_deg)
        ops._angle_rad(self.sigma_deg, "sigma_deg")   # raises unless finite and >= 0
        ops._angle_rad(self.max_angle_deg, "max_angle_deg", allow_none=True)
        if motion not in ("walk", "constant_velocity"):
            raise RuntimeError("motion = %r: expected 'walk' or 'constant_velocity'" % (motion,))
        self.motion = motion
        self.sigma_vel_deg, self.damping, self.coast = float(sigma_vel_deg), float(damping), bool(coast)
        self.max_speed_deg = None if max_speed_deg is None else float(max_speed_deg)
        ops._angle_rad(self.sigma_vel_deg, "sigma_vel_deg")
        ops._angle_rad(self.max_speed_deg, "max_speed_deg", allow_none=True)
        ops._unit_interval(self.damping, "damping")
        self.temperature = float(temperature)
        ops.inverse_temperature(self.temperature)     # raises unless finite and > 0
        if adapt is not None:
            if not self.sigma_deg > 0.0:
                raise RuntimeError("adapt= needs sigma_deg > 0 (sigma_vel follows sigma / sigma_deg), got %r" % (sigma_deg,))
            self._n_fresh_lost = self.n_fresh if adapt.n_fresh_lost is None else adapt.n_fresh_lost
            if not 0 <= self._n_fresh_lost <= self.M:
                raise RuntimeError("n_fresh_lost = %d outside 0..particles = %d" % (self._n_fresh_lost, self.M))
        self.history = int(history)
        if self.history != 0 and not 2 <= self.history < (1 << 31):
            raise RuntimeError("history = %d: 0 (no smoothing) or at least 2 frames" % self.history)
        if self.history and not (hasattr(self.ops, "smooth_step") and hasattr(self.ops, "smooth_backtrace")):
            raise RuntimeError("history = %d needs a backend that provides smooth_step and smooth_backtrace" % self.history)
        if smooth_sigma_deg is None:
            smooth_sigma_deg = self.sigma_deg if motion == "walk" else math.hypot(self.sigma_deg, self.sigma_vel_deg)
        self.smooth_sigma_deg, self.smooth_jump = float(smooth_sigma_deg), ops._jump(smooth_jump)
        if self.history and not ops._angle_rad(self.smooth_sigma_deg, "smooth_sigma_deg") > 0.0:
            raise RuntimeError("smooth_sigma_deg = %r must be > 0" % (smooth_sigma_deg,))
        self.marginals = bool(marginals)
        if self.marginals and not self.history:
            raise RuntimeError("marginals=True needs history >= 2: the marginals are computed over the smoother's ring")
        if self.marginals and not (hasattr(self.ops, "marginal_step") and hasattr(self.ops, "marginal_smooth")):
            raise RuntimeError("marginals=True needs a backend that provides marginal_step and marginal_smooth")
        self.seed = int(seed)
        self.posterior = bool(posterior)
        self.mode_angle_deg = float(mode_angle_deg)
        if self.posterior:
            ops.min_trace(self.mode_angle_deg)        # raises outside (0, 180)
        hip = backend is None and dev.type == "cuda"
        if use_graph and not hip:
            raise RuntimeError("use_graph=True needs the HIP backend on a GPU (backend=None, weights on the device)")
        self.use_graph = bool(use_graph)
        B, M = self.B, self.M
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        self._R = [f(B, M, 3, 3) for _ in range(2)]
        self._V = [torch.zeros((B, M, 3), dtype=torch.float32, device=dev) for _ in range(2)] if motion != "walk" else None
        self._vel = None      # the velocities of the set the next step draws from (None: zeros)
        self._scores = [f(B, M) for _ in range(2)]
        self._keys = [torch.full((B,), KEY_EMPTY, dtype=torch.int64, device=dev) for _ in range(2)]
        self._sel = [(f(B), torch.empty((B,), dtype=torch.int64, device=dev), f(B, 3, 3)) for _ in range(2)]
        self._reacq = [torch.zeros((B,), dtype=torch.bool, device=dev) for _ in range(2)]
        self._draws = torch.full((B, M), -1, dtype=torch.int64, device=dev)
        self._u = f(B)
        self._step = torch.zeros((1,), dtype=torch.int64, device=dev)
        self._ws = ops.resample_workspace(B, M, dev) if hip else None      # steady state: draws from an M-sized set
        self._ws0 = None                                                   # first step: draws from the N0-sized set
        self._pstate = ops.pose_posterior_state(B, 1, dev) if hip and self.posterior else None
        self._pws = ops.pose_posterior_workspace(B, M, 1, dev) if hip and self.posterior else None
        # the smoother's ring (any backend: plain tensors); after init the counter is 0 and the first step records frame 1
        self._hist = ops.smooth_history(B, M, self.history, dev, velocities=motion != "walk") if self.history else None
        self._marg = ops.marginal_history(B, M, self.history, dev) if self.marginals else None
        # the control record (adapt): what the next predict step reads; init copies _ctl0 into it
        self._ctl0 = ops.track_control_state(B, self.sigma_deg, self.sigma_vel_deg if motion != "walk" else 0.0, self.n_fresh,
                                             dev) if adapt is not None else None
        self._ctl = self._ctl0.clone() if adapt is not None else None
        self._cur = None      # (R, scores, key) of the set the next step draws from
        self._anchor = None   # (B,3,3): the previous frame's MAP pose, the anchor of the fold (symmetry)
        self._n = 0           # steps since init
        self._static = None
        self._selected = False    # select_views() since the last step (views)
        self._graphs = {}     # half of the ping-pong (views: and whether the step selects and gathers) -> (graph, its TrackStep)
        if views is not None:
            A = views.detach().to(device=dev, dtype=torch.float32)
            self.views = (A[None].expand(B, self.V, 3, 3) if A.dim() == 3 else A).contiguous()
            K = self.K
            self._vsel = ops.ViewSelection(torch.zeros((B, K), dtype=torch.int32, device=dev), f(B, K, 3, 3))
            self._vws = ops.verify_views_workspace(B, K, M, dev) if hip else None
            self._full = None        # the static (B,V,...) inputs of a captured step that selects and gathers

    @property
    def buffers(self):
        """The static input volumes ``(vol_src, vol_tgt)`` of the captured step (allocated on first use); with ``views`` the
        staged volumes ``(refs (B,K,16,8,8,8), query (B,K,16,8,8,8))`` of every step."""
        if self._static is None:
            lead = (self.B,) if self.views is None else (self.B, self.K)
            self._static = tuple(torch.zeros(lead + (16, 8, 8, 8), dtype=torch.float32, device=self.W1.device) for _ in range(2))
        return self._static

    @property
    def view_selection(self):
        """``ops.ViewSelection(idx (B,K) int32, A (B,K,3,3))``: the views the last step scored against, or -- after
        ``select_views()`` -- the ones the next step will.  Buffers the tracker owns (None without ``views``)."""
        return self._vsel if self.views is not None else None

    @property
    def view_inputs(self):
        """The static ``(vol_refs (B,V,...), vol_query)`` of the captured step that selects and gathers (``use_graph=True``
        with ``views``): allocated, in the shapes given, by the first such step after the eager one; None before.  Write the
        frame's volumes there and pass the two tensors themselves to ``step`` to replay with no staging copy."""
        return self._full if self.views is not None else None

    @torch.no_grad()
    def select_views(self):
        """Pick the ``views_per_step`` views nearest the current MAP pose: ONE launch, the anchor read on the device.  Returns
        the ``ViewSelection`` the next step uses (gather the K references' inputs by its ``idx``)."""
        if self.views is None:
            raise RuntimeError("select_views() needs a tracker built with views=")
        if self._cur is None:
            raise RuntimeError("call init(vol_refs, vol_query, R_init) before select_views()")
        self.ops.nearest_views(self._anchor, self.views, self.K, out=self._vsel)
        self._selected = True
        return self._vsel

    @property
    def control_record(self) -> Optional[torch.Tensor]:
        """The raw control record ``(B,8)`` int32 (``adapt``; None without): what the next step's predict reads."""
        return self._ctl

    def control(self):
        """The control record decoded ON THE HOST (``ops.decode_track_control``: it synchronises): sigma, sigma_vel and n_fresh
        of the next step, and lost / reacquired / updated, the innovation and the score of the last one."""
        if self._ctl is None:
            raise RuntimeError("control() needs a tracker built with adapt=")
        return ops.decode_track_control(self._ctl)

    @property
    def step_counter(self) -> torch.Tensor:
        """The int64 device counter (one element): 0 after ``init``, moved by one per step ON THE DEVICE."""
        return self._step

    @property
    def velocities(self) -> Optional[torch.Tensor]:
        """``(B,M,3)`` float32: the velocities of the current particles (``motion="constant_velocity"``, after a step); None
        after ``init`` (the scored set has none) and with ``motion="walk"``."""
        return self._vel

    def _posterior(self, scores, R, R_map, state=None, workspace=None):
        if not self.posterior:
            return None, None, None, None
        p = self.ops.pose_posterior(scores, R, self.temperature, anchors=R_map[:, None], min_angle_deg=self.mode_angle_deg,
                                    state=state, workspace=workspace, reset=True if state is not None else None)
        return p.R_mean, p.spread_deg, p.mode_prob[:, 0], p.entropy

    @torch.no_grad()
    def init(self, vol_src: torch.Tensor, vol_tgt: torch.Tensor, R_init: torch.Tensor) -> TrackStep:
        """Score ``R_init (N0,3,3)`` / ``(B,N0,3,3)`` on the pair: the set, with its scores, that the first step draws from.
        Restarts the step counter at 0, so a trajectory is a function of (seed, inputs)."""
        o = self.ops
        if R_init.dim() not in (3, 4) or tuple(R_init.shape[-2:]) != (3, 3) or (R_init.dim() == 4 and R_init.shape[0] != self.B):
            raise RuntimeError("R_init must be (N0,3,3) or (B,N0,3,3) with B = %d, got %s" % (self.B, tuple(R_init.shape)))
        if vol_src.shape[0] != self.B:
            raise RuntimeError("the tracker was built for batch = %d, got volumes %s" % (self.B, tuple(vol_src.shape)))
        R0 = R_init.detach().clone(memory_format=torch.contiguous_format)   # the first step reads it: keep a copy of our own
        if self.views is None:
            scores, key = o.verify_pair(vol_src, vol_tgt, R0, self.W1, self.W2, self.b2, want_scores=True)
        else:   # densely over all V views
            scores, key = o.verify_views_staged(vol_src, vol_tgt, R0, self.views, self.W1, self.W2, self.b2,
                                                max_view_angle_deg=self.max_view_angle_deg)
            self._selected = False
        score, idx, R_map = o.select_rotation(key, R0)
        n0 = R0.shape[-3]
        if self.ops is ops and R0.is_cuda and (self._ws0 is None or self._ws0_n != n0):
            self._ws0, self._ws0_n = ops.resample_workspace(self.B, n0, R0.device), n0
        self._step.zero_()
        if self._ctl is not None:
            self._ctl.copy_(self._ctl0)
        self._cur, self._n, self._vel = (R0, scores, key), 0, None
        self._anchor = R_map   # the pose the next step folds around (symmetry)
        post = self._posterior(scores, R0, R_map)
        return TrackStep(score, idx, R_map, R0, scores, None, *post, torch.zeros_like(idx, dtype=torch.bool))

    def _run(self, vol_src, vol_tgt, p: int) -> TrackStep:
        """One step into half ``p`` of the buffers; runs eagerly or under capture."""
        o = self.ops
        R_prev, s_prev, key_prev = self._cur
        ws = self._ws if R_prev.shape[-3] == self.M and R_prev is self._R[1 - p] else self._ws0
        u = o.track_advance(self._step, self.seed, self.B, u=self._u)
        draws = o.resample(s_prev, self.M, self.temperature, u=u, out=self._draws, workspace=ws)
        first = 1
        if self.adapt is not None:   # sigma, sigma_vel and n_fresh come from the record, on the device
            cv = self.motion != "walk"
            first = 2 if cv and self.coast else 1
            R = o.predict_rotations_controlled(R_prev, self._ctl, self._vel, idx=draws, damping=self.damping if cv else 1.0,
                                               step=self._step, seed=self.seed, best_key=key_prev, coast=cv and self.coast,
                                               max_angle_deg=self.max_angle_deg, max_speed_deg=self.max_speed_deg if cv else None,
                                               out=self._R[p], vel_out=self._V[p] if cv else None, velocities=cv)
            R = R[0] if cv else R
        elif self.motion == "walk":
            R = o.diffuse_rotations(R_prev, idx=draws, sigma_deg=self.sigma_deg, step=self._step, seed=self.seed,
                                    best_key=key_prev, n_fresh=self.n_fresh, max_angle_deg=self.max_angle_deg, out=self._R[p])
        else:
            R, _ = o.predict_rotations(R_prev, self._vel, idx=draws, sigma_deg=self.sigma_deg, sigma_vel_deg=self.sigma_vel_deg,
                                       damping=self.damping, step=self._step, seed=self.seed, best_key=key_prev, coast=self.coast,
                                       n_fresh=self.n_fresh, max_angle_deg=self.max_angle_deg, max_speed_deg=self.max_speed_deg,
                                       out=self._R[p], vel_out=self._V[p])
            first = 2 if self.coast else 1
        if self.symmetry is not None:   # in place: one fundamental domain around the previous MAP pose; the elite slots are kept
            V = self._V[p] if self._V is not None else None
            o.sym_fold(R, self.symmetry, self._anchor[:, None], None, keep=min(first, self.M), V=V, out=R, V_out=V, want_info=False)
        if self.views is None:
            scores, key = o.verify_pair(vol_src, vol_tgt, R, self.W1, self.W2, self.b2, want_scores=True, best_key=self._keys[p],
                                        reset_best=True, scores_out=self._scores[p])
        else:   # (vol_src, vol_tgt) are the K staged views' volumes, self._vsel.A their rotations
            scores, key = o.verify_views_staged(vol_src, vol_tgt, R, self._vsel.A, self.W1, self.W2, self.b2,
                                                max_view_angle_deg=self.max_view_angle_deg, workspace=self._vws,
                                                scores_out=self._scores[p], best_key=self._keys[p], reset_best=True)
        score, idx, R_map = o.select_rotation(key, R, out=self._sel[p])
        # the winner sits in a fresh slot (slot 0 is the elite, and slot 1 the coasting one, even when every slot is fresh)
        if self.adapt is None:
            reacq = torch.ge(idx, max(self.M - self.n_fresh, first), out=self._reacq[p])
        else:   # the same comparison against the n_fresh this frame used, and the record of the next frame
            a = self.adapt
            reacq = o.track_control(self._ctl, R, idx, score, V=self._V[p] if self._V is not None else None, first=first,
                                    sigma_deg=self.sigma_deg, sigma_vel_deg=self.sigma_vel_deg if self._V is not None else 0.0,
                                    n_fresh=self.n_fresh, sigma_min_deg=a.sigma_min_deg, sigma_max_deg=a.sigma_max_deg, gain=a.gain,
                                    rate=a.rate, score_floor=a.score_floor, n_fresh_lost=self._n_fresh_lost,
                                    reacquired=self._reacq[p])
        post = self._posterior(scores, R, R_map, self._pstate, self._pws)
        if self._hist is not None:   # observes the step, changes none of its outputs
            o.smooth_step(self._hist, R, scores, self._step, self.temperature, self.smooth_sigma_deg, jump=self.smooth_jump,
                          V=self._V[p] if self._V is not None else None, damping=self.damping, first_step=1)
            if self._marg is not None:
                o.marginal_step(self._hist, self._marg, R, scores, self._step, self.temperature, self.smooth_sigma_deg,
                                jump=self.smooth_jump, first_step=1)
        return TrackStep(score, idx, R_map, R, scores, draws, *post, reacq)

    def _frames(self, frames: Optional[int], what: str) -> int:
        """F of a smoothing query: ``min(frames, steps since init, history)``, ``frames`` None standing for no limit."""
        if self._n < 1:
            raise RuntimeError("%s before the first step: nothing has been recorded since init" % what)
        F = min(self._n, self.history)
        if frames is not None:
            if int(frames) < 1:
                raise RuntimeError("frames = %d must be at least 1" % int(frames))
            F = min(F, int(frames))
        return F

    @torch.no_grad()
    def smoothed(self, frames: Optional[int] = None, out=None):
        """The MAP trajectory over the last ``min(frames, steps since init, history)`` frames (``frames`` None: as many as there
        are): ``ops.SmoothedPath(idx (B,F) int64, R (B,F,3,3))``, oldest first, the last column the current frame.  One launch,
        no host synchronisation; ``out``: a ``SmoothedPath`` of that size to write into."""
        if self._hist is None:
            raise RuntimeError("smoothed() needs a tracker built with history >= 2")
        return self.ops.smooth_backtrace(self._hist, self._step, frames=self._frames(frames, "smoothed()"), first_step=1, out=out)

    @torch.no_grad()
    def smoothed_marginals(self, frames: Optional[int] = None, out=None, posterior: bool = False):
        """The smoothed marginals over the last ``min(frames, steps since init, history)`` frames:
        ``ops.SmoothedMarginals(logw (B,F,M), idx (B,F) int64, R (B,F,3,3))``, oldest first, the last column the current frame
        (where the marginal is the filter's own posterior).  ``logw[b,f]`` is the log-probability that the trajectory passes
        through each particle of that frame given all F frames, ``idx`` its first arg-max and ``R`` that particle's pose.  F
        launches, no host synchronisation; ``out``: a ``SmoothedMarginals`` of that size to write into.
        ``posterior=True``: returns ``(marginals, R_mean (B,F,3,3), spread_deg, mode_mass, entropy (B,F))`` -- every frame's
        row and particle set through ``pose_posterior`` at ``temperature=1`` with the frame's ``R`` as the single anchor and
        ``mode_angle_deg``, as one batch of B F rows: the smoothed mean pose, its spread, the mass within ``mode_angle_deg`` of
        the most probable particle and the entropy in nats.  The query gathers the frames from the ring and allocates."""
        if self._marg is None:
            raise RuntimeError("smoothed_marginals() needs a tracker built with history >= 2 and marginals=True")
        F = self._frames(frames, "smoothed_marginals()")
        if posterior:
            ops.min_trace(self.mode_angle_deg)        # raises outside (0, 180), before any launch
        res = self.ops.marginal_smooth(self._hist, self._marg, self._step, self.smooth_sigma_deg, jump=self.smooth_jump, frames=F,
                                       first_step=1, out=out)
        if not posterior:
            return res
        B, M = self.B, self.M
        # the counter is 0 after init and moves by one per step: frame n lives in slot n mod H
        slots = torch.tensor([(self._n - F + 1 + f) % self.history for f in range(F)], dtype=torch.int64, device=res.logw.device)
        sets = self._hist.R.index_select(0, slots).transpose(0, 1).reshape(B * F, M, 3, 3)
        p = self.ops.pose_posterior(res.logw.reshape(B * F, M), sets, 1.0, anchors=res.R.reshape(B * F, 1, 3, 3),
                                    min_angle_deg=self.mode_angle_deg)
        return (res, p.R_mean.reshape(B, F, 3, 3), p.spread_deg.reshape(B, F), p.mode_prob[:, 0].reshape(B, F),
                p.entropy.reshape(B, F))

    def _run_views(self, vol_refs, vol_query, p: int) -> TrackStep:
        """One step of a tracker with views from ``(B,V,...)`` inputs: select, gather into the staged buffers, the chain."""
        o = self.ops
        vol_refs, vol_query = vol_refs.detach().contiguous(), vol_query.detach().contiguous()
        sel = o.nearest_views(self._anchor, self.views, self.K, out=self._vsel)
        refs, query = self.buffers
        o.gather_views(vol_refs, sel.idx, out=refs)
        o.gather_views(vol_query, sel.idx, out=query, broadcast=vol_query.dim() == 5)
        return self._run(refs, query, p)

    def _step_views(self, vol_refs, vol_query, staged: bool) -> TrackStep:
        B, V, K = self.B, self.V, self.K
        vol = (16, 8, 8, 8)
        staged = staged or vol_refs is None
        if staged:
            if not self._selected:
                raise RuntimeError("a staged step scores against the views of select_views(): call it after the last step "
                                   "(and gather the inputs by its idx)")
            if vol_refs is not None and (tuple(vol_refs.shape) != (B, K) + vol or tuple(vol_query.shape) != (B, K) + vol):
                raise RuntimeError("staged volumes must both be (B,K,16,8,8,8) = %s, got %s and %s"
                                   % ((B, K) + vol, tuple(vol_refs.shape), tuple(vol_query.shape)))
        elif tuple(vol_refs.shape) != (B, V) + vol or tuple(vol_query.shape) not in ((B,) + vol, (B, V) + vol):
            raise RuntimeError("vol_refs must be (B,V,16,8,8,8) = %s and vol_query that or (B,16,8,8,8), got %s and %s"
                               % ((B, V) + vol, tuple(vol_refs.shape), tuple(vol_query.shape)))
        if staged:
            return self._advance((vol_refs, vol_query), lambda: self.buffers, self._run, lambda p: (p, True))
        return self._advance((vol_refs, vol_query), lambda: self._view_statics(vol_refs, vol_query), self._run_views,
                             lambda p: (p, False))

    def _view_statics(self, vol_refs, vol_query):
        """The static ``(B,V,...)`` inputs of the captured step that selects and gathers, in the shapes given."""
        if self._full is None or self._full[1].shape != vol_query.shape:
            self._full = (torch.empty_like(vol_refs, memory_format=torch.contiguous_format),
                          torch.empty_like(vol_query, memory_format=torch.contiguous_format))
            self._graphs = {k: g for k, g in self._graphs.items() if k[1]}   # (graphs of the old inputs' shape)
        return self._full

    def _advance(self, vols, static, run, key) -> TrackStep:
        """One step through ``run(vol_a, vol_b, p)``: eagerly on ``vols`` (``static()`` when none are given), or -- ``use_graph``,
        past the first step -- captured once per ``key(p)`` on the inputs ``static()`` and replayed; then the ping-pong moves."""
        n = self._n + 1
        p = n & 1
        if not self.use_graph or n == 1:
            out = run(*(vols if vols[0] is not None else static()), p)
        else:
            st = static()
            for dst, src in zip(st, vols):
                if src is not None and src.data_ptr() != dst.data_ptr():
                    dst.copy_(src)
            k = key(p)
            if k not in self._graphs:
                # No warm-up run: the eager first step has issued every launch of the chain once, and a warm-up here would
                # move the filter (the counter, the sets).  Capture records the step; the replay below runs it.
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    captured = run(st[0], st[1], p)
                self._graphs[k] = (graph, captured)
            graph, out = self._graphs[k]
            graph.replay()
        self._cur, self._n = (self._R[p], self._scores[p], self._keys[p]), n
        self._anchor = self._sel[p][2]
        self._selected = False
        if self._V is not None:
            self._vel = self._V[p]
        return out

    @torch.no_grad()
    def step(self, vol_src: Optional[torch.Tensor] = None, vol_tgt: Optional[torch.Tensor] = None, staged: bool = False) -> TrackStep:
        """Advance the filter by one frame.  Called with no volumes it runs on ``self.buffers`` as they are.  With ``views``:
        ``(B,V,...)`` inputs are selected from and gathered; ``staged=True`` (or no volumes) runs on the K staged views."""
        if self._cur is None:
            raise RuntimeError("call init(vol_src, vol_tgt, R_init) before the first step")
        if (vol_src is None) != (vol_tgt is None):
            raise RuntimeError("pass both volumes or neither")
        if self.views is not None:
            return self._step_views(vol_src, vol_tgt, staged)
        if staged:
            raise RuntimeError("staged=True belongs to a tracker built with views=")
        return self._advance((vol_src, vol_tgt), lambda: self.buffers, self._run, lambda p: p)
