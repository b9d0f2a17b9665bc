"""Rotation-hypothesis generators and the angular error metric (host side).

The reference draws hypotheses with ``pytorch3d.transforms.random_rotations``
(test_co3d.py:106, test_linemod.py:43, modules/model.py:184) -- third-party code
that is not in the reference tree.  Only the *distribution* (Haar-uniform on
SO(3)) matters: hypotheses are inputs of the hot path, not results.  These are
our own samplers: normalised Gaussian quaternions, a deterministic
super-Fibonacci SO(3) grid (BASELINE.json config 3; no grid exists in the
reference) and a local refinement sampler (config 5).
"""
from __future__ import annotations

import math

import numpy as np
import torch


def quaternion_to_matrix_np(q: np.ndarray) -> np.ndarray:
    """(n,4) real-first quaternions (any norm > 0) -> (n,3,3) rotation matrices, float64 maths."""
    q = np.asarray(q, dtype=np.float64)
    r, i, j, k = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    s = 2.0 / (q * q).sum(axis=1)
    m = np.stack(
        [
            1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r),
            s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r),
            s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j),
        ],
        axis=1,
    )
    return m.reshape(-1, 3, 3)


def haar_rotations_np(n: int, seed: int) -> np.ndarray:
    """n Haar-uniform rotations, float32 (n,3,3); bit-reproducible from `seed`.

    Uses numpy's frozen legacy RandomState stream so that tests on any box can
    regenerate the exact hypothesis set whose SHA-256 is stored in the golden
    fixtures.
    """
    rs = np.random.RandomState(seed)
    q = rs.standard_normal(size=(n, 4))
    return quaternion_to_matrix_np(q).astype(np.float32)


def random_rotations(n: int, dtype=torch.float32, device=None, generator: torch.Generator | None = None):
    """Drop-in for ``pytorch3d.transforms.random_rotations(n)``: Haar-uniform (n,3,3)."""
    q = torch.randn((n, 4), dtype=torch.float64, device=device, generator=generator)
    r, i, j, k = q.unbind(-1)
    s = 2.0 / (q * q).sum(-1)
    m = torch.stack(
        [
            1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r),
            s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r),
            s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j),
        ],
        dim=-1,
    )
    return m.reshape(n, 3, 3).to(dtype)


def _sincos_turns(f: np.ndarray):
    """sin(2 pi f), cos(2 pi f) for f in [0, 1) from +, -, * alone (nearest octant + Taylor series on |x| <= pi/8):
    correct to ~1e-16 and, unlike libm / SIMD sin and cos, bit-reproducible on every IEEE-754 machine -- the SHA-256 of
    the grid is stored in a golden fixture and re-derived on another box."""
    f = np.asarray(f, dtype=np.float64)
    k = np.floor(f * 8.0 + 0.5)
    x = (f - k * 0.125) * (2.0 * math.pi)
    x2 = x * x
    sn = np.ones_like(x)
    cs = np.ones_like(x)
    for m in range(9, 0, -1):  # Horner: sin x = x (1 - x2/(2.3) (1 - x2/(4.5) ...)), cos x = 1 - x2/(1.2) (1 - x2/(3.4) ...)
        sn = 1.0 - sn * x2 * (1.0 / ((2 * m) * (2 * m + 1)))
        cs = 1.0 - cs * x2 * (1.0 / ((2 * m - 1) * (2 * m)))
    sn = sn * x
    h = math.sqrt(0.5)
    tab_s = np.array([0.0, h, 1.0, h, 0.0, -h, -1.0, -h])
    tab_c = np.array([1.0, h, 0.0, -h, -1.0, -h, 0.0, h])
    ki = k.astype(np.int64) & 7
    s0, c0 = tab_s[ki], tab_c[ki]
    return s0 * cs + c0 * sn, c0 * cs - s0 * sn


def so3_grid_np(n: int) -> np.ndarray:
    """Deterministic, nearly uniform SO(3) grid of n rotations (super-Fibonacci spiral).

    Build-defined (the reference has no grid: test_linemod.py:43 samples randomly).
    Alexa, "Super-Fibonacci Spirals: Fast, Low-Discrepancy Sampling of SO(3)", CVPR 2022.
    Point i is the quaternion (sqrt(t) sin a, sqrt(t) cos a, sqrt(1-t) sin b, sqrt(1-t) cos b) with t = (i + 1/2)/n,
    a = 2 pi (i + 1/2)/sqrt(2), b = 2 pi (i + 1/2)/psi; the angles are reduced as turn fractions first (they reach
    10^6 rad) and sin / cos come from ``_sincos_turns``, so the float32 result is the same bytes on every machine.
    """
    psi = 1.533751168755204288118041
    i = np.arange(n, dtype=np.float64)
    s = i + 0.5
    t = s / n
    fa, fb = s * math.sqrt(0.5), s * (1.0 / psi)
    fa, fb = fa - np.floor(fa), fb - np.floor(fb)
    r, R = np.sqrt(t), np.sqrt(1.0 - t)
    sa, ca = _sincos_turns(fa)
    sb, cb = _sincos_turns(fb)
    q = np.stack([r * sa, r * ca, R * sb, R * cb], axis=1)
    return quaternion_to_matrix_np(q).astype(np.float32)


def axis_angle_to_matrix(omega: torch.Tensor) -> torch.Tensor:
    """Rodrigues: (n,3) rotation vectors -> (n,3,3)."""
    theta = omega.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    k = omega / theta
    K = omega.new_zeros(omega.shape[0], 3, 3)
    K[:, 0, 1], K[:, 0, 2] = -k[:, 2], k[:, 1]
    K[:, 1, 0], K[:, 1, 2] = k[:, 2], -k[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -k[:, 1], k[:, 0]
    st, ct = torch.sin(theta)[..., None], torch.cos(theta)[..., None]
    eye = torch.eye(3, dtype=omega.dtype, device=omega.device)[None]
    return eye + st * K + (1 - ct) * (K @ K)


def refine_rotations(R_star: torch.Tensor, n: int, max_angle_deg: float, generator=None) -> torch.Tensor:
    """Local refinement set around R_star (3,3): R_star @ exp([w]x), |w| <= max_angle (config 5).

    Index 0 is R_star itself so that refinement can never lower the best score.
    """
    dev = R_star.device
    v = torch.randn((n, 3), dtype=torch.float64, device=dev, generator=generator)
    v = v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    # uniform in the ball of rotation vectors: radius ~ U^(1/3)
    rad = torch.rand((n, 1), dtype=torch.float64, device=dev, generator=generator) ** (1.0 / 3.0)
    w = v * rad * math.radians(max_angle_deg)
    w[0] = 0
    return (R_star.to(torch.float64)[None] @ axis_angle_to_matrix(w)).to(R_star.dtype)


def geodesic_deg(R_pred: torch.Tensor, R_gt: torch.Tensor) -> torch.Tensor:
    """Angular error in degrees, exactly the reference's expression (test_co3d.py:149-150,
    modules/model.py:199-200, test_linemod.py:66-67): arccos(((sum(Rp*Rg)).clamp(-1,3)-1)/2)*180/pi."""
    sim = (torch.sum(R_pred.reshape(-1, 9) * R_gt.reshape(-1, 9), dim=-1).clamp(-1, 3) - 1) / 2
    return torch.arccos(sim) * 180.0 / math.pi


# ---- SO(3) ascent step: the host statement of ahv_so3_ascent_candidates_f32 / ahv_so3_ascent_select_f32 ----------------
# (what the CPU tests execute and the GPU tests compare the kernels with; ``ops`` never falls back to it)

def so3_tangent(R: torch.Tensor, G: torch.Tensor) -> torch.Tensor:
    """The skew part ``1/2 (R^T G - G^T R)`` of ``R^T G`` (..., 3, 3): the Riemannian gradient of a function with Euclidean
    gradient ``G`` at ``R``, in the body frame -- d/de f(R exp(e [w]x)) = 2 <vee(.), w>."""
    A = R.transpose(-1, -2) @ G
    return 0.5 * (A - A.transpose(-1, -2))


def so3_ascent_candidates(R_cur: torch.Tensor, grad_R: torch.Tensor, theta: torch.Tensor, ladder) -> torch.Tensor:
    """``R_cur, grad_R (B,K,3,3)``, ``theta (B,K)`` radians, ``ladder`` L factors -> ``(B, K*(L+1), 3, 3)``: slot 0 of a seed is
    ``R_cur`` itself, slot ``l >= 1`` is ``R_cur exp(ladder[l-1] theta [w/|w|]x)`` with ``w = vee(so3_tangent(R_cur, grad_R))``;
    ``|w| = 0`` or a non-finite ``w``: every slot is ``R_cur``."""
    B, K = R_cur.shape[:2]
    ladder = torch.as_tensor(ladder, dtype=R_cur.dtype, device=R_cur.device).reshape(-1)
    L = ladder.numel()
    S = so3_tangent(R_cur, grad_R)
    w = torch.stack([S[..., 2, 1], S[..., 0, 2], S[..., 1, 0]], dim=-1)
    nrm = (w * w).sum(-1).sqrt()
    move = (nrm > 0) & torch.isfinite(nrm)
    n = torch.where(move[..., None], w / torch.where(move, nrm, torch.ones_like(nrm))[..., None], torch.zeros_like(w))
    a = theta[..., None] * ladder                                   # (B,K,L)
    sn, c1 = torch.sin(a)[..., None, None], (2 * torch.sin(0.5 * a) ** 2)[..., None, None]
    Kx = torch.zeros_like(R_cur)
    Kx[..., 0, 1], Kx[..., 0, 2] = -n[..., 2], n[..., 1]
    Kx[..., 1, 0], Kx[..., 1, 2] = n[..., 2], -n[..., 0]
    Kx[..., 2, 0], Kx[..., 2, 1] = -n[..., 1], n[..., 0]
    eye = torch.eye(3, dtype=R_cur.dtype, device=R_cur.device)
    nnT = n[..., :, None] * n[..., None, :]
    E = eye + sn * Kx[:, :, None] + c1 * (nnT - eye)[:, :, None]   # (B,K,L,3,3)
    moved = R_cur[:, :, None] @ E
    stay = R_cur[:, :, None].expand(B, K, L, 3, 3)
    cand = torch.where(move[..., None, None, None], moved, stay)
    return torch.cat([R_cur[:, :, None], cand], dim=2).reshape(B, K * (L + 1), 3, 3)


def so3_ascent_select(R_cand: torch.Tensor, cand_scores: torch.Tensor, theta: torch.Tensor, ladder):
    """``R_cand (B, K*(L+1), 3, 3)``, its scores ``(B, K*(L+1))`` -> ``(R_cur (B,K,3,3), score_cur (B,K), theta (B,K))``.  Slots
    are scanned in order and a candidate replaces the incumbent only if its score is strictly greater (false for NaN): a
    seed's score never decreases, slot 0 wins ties.  ``theta <- ladder[l-1] theta`` for the accepted slot, ``theta min(ladder)``
    when slot 0 stayed."""
    B, K = theta.shape
    ladder = torch.as_tensor(ladder, dtype=theta.dtype, device=theta.device).reshape(-1)
    L = ladder.numel()
    sc = cand_scores.reshape(B, K, L + 1)
    best = sc[..., 0].clone()
    slot = torch.zeros((B, K), dtype=torch.int64, device=sc.device)
    for l in range(1, L + 1):
        better = sc[..., l] > best
        best = torch.where(better, sc[..., l], best)
        slot = torch.where(better, torch.full_like(slot, l), slot)
    Rc = R_cand.reshape(B, K, L + 1, 3, 3)
    R_new = torch.gather(Rc, 2, slot[..., None, None, None].expand(B, K, 1, 3, 3))[:, :, 0]
    factor = torch.cat([ladder.min().reshape(1), ladder])[slot]
    return R_new, best, theta * factor


# ---- symmetric objects: pose selection modulo a symmetry group ------------------------------------------------------------
# Hypotheses are relative rotations R (source view -> target view); the object's symmetry group, written in the SOURCE VIEW'S
# frame, acts on the right: R and R S are the same pose.  With the group G0 in the object's own frame and the source view's
# object-to-camera rotation P the group is P G0 P^T (R = P_t P_s^T, whose alternatives are P_t S P_s^T = R (P_s S P_s^T)).

SYM_MAX_ELEMENTS = 64
SYM_TOL = 1e-5   # Frobenius: the fp32 rounding of a product of two exact group elements is ~3e-7


def _unit(axis) -> np.ndarray:
    if isinstance(axis, str):
        axis = {"X": (1.0, 0.0, 0.0), "Y": (0.0, 1.0, 0.0), "Z": (0.0, 0.0, 1.0)}[axis.upper()]
    a = np.asarray(axis, dtype=np.float64).reshape(3)
    n = float(np.linalg.norm(a))
    if not n > 0.0:
        raise ValueError("axis must be non-zero")
    return a / n


def _rot_np(axis: np.ndarray, angle: float) -> np.ndarray:
    """Rodrigues in fp64: cos I + sin [a]x + (1 - cos) a a^T; quarter turns give exact 0 / +-1 entries."""
    q = angle / (0.5 * math.pi)
    if abs(q - round(q)) < 1e-12:
        c, s = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][int(round(q)) % 4]
    else:
        c, s = math.cos(angle), math.sin(angle)
    a = axis
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return c * np.eye(3) + s * K + (1.0 - c) * np.outer(a, a)


def _perp(a: np.ndarray) -> np.ndarray:
    """A unit vector perpendicular to a (deterministic)."""
    e = np.zeros(3)
    e[int(np.argmin(np.abs(a)))] = 1.0
    p = np.cross(a, e)
    return p / np.linalg.norm(p)


def _closure(gens) -> np.ndarray:
    """The group generated by ``gens`` (fp64), identity first, in order of discovery (breadth first)."""
    elems = [np.eye(3)]
    frontier = [np.eye(3)]
    while frontier:
        nxt = []
        for e in frontier:
            for g in gens:
                c = e @ g
                if not any(np.abs(c - x).max() < 1e-9 for x in elems):
                    if len(elems) >= SYM_MAX_ELEMENTS:
                        raise ValueError("the generators span more than %d elements" % SYM_MAX_ELEMENTS)
                    elems.append(c)
                    nxt.append(c)
        frontier = nxt
    return np.stack(elems)


class Symmetry:
    """A symmetry group in the source view's frame: ``S (G,3,3)`` or ``(B,G,3,3)`` float32, 1 <= G <= 64, ``S[..., 0, :, :]`` the
    identity exactly, closed under product and inverse; optionally a continuous ``axis (3,)`` / ``(B,3)`` (unit) about which every
    rotation is a symmetry too -- every ``S[g]`` must then map the axis to +- itself.  G = 1 with an axis is C_inf, G = 2 with a
    flip D_inf.  The constructor checks all of this to a Frobenius tolerance of 1e-5.  Construction is fp64 rounded to fp32."""

    def __init__(self, S, axis=None):
        S = torch.as_tensor(S)
        if S.dim() not in (3, 4) or tuple(S.shape[-2:]) != (3, 3):
            raise ValueError("S must be (G,3,3) or (B,G,3,3), got %s" % (tuple(S.shape),))
        G = S.shape[-3]
        if not 1 <= G <= SYM_MAX_ELEMENTS:
            raise ValueError("G = %d outside 1..%d" % (G, SYM_MAX_ELEMENTS))
        self.S = S.to(torch.float32).contiguous()
        self.axis = None
        if axis is not None:
            axis = torch.as_tensor(axis).to(torch.float32).contiguous()
            if tuple(axis.shape) != (3,) and not (axis.dim() == 2 and axis.shape[1] == 3):
                raise ValueError("axis must be (3,) or (B,3), got %s" % (tuple(axis.shape),))
            if axis.dim() == 2 and S.dim() == 4 and axis.shape[0] != S.shape[0]:
                raise ValueError("S and axis disagree on B")
            self.axis = axis
        self._check()

    def _check(self):
        S = self.S.detach().cpu().to(torch.float64).reshape(-1, self.order, 3, 3)
        eye = torch.eye(3, dtype=torch.float64)
        if not bool((self.S.detach().cpu().reshape(-1, self.order, 3, 3)[:, 0] == torch.eye(3)).all()):
            raise ValueError("S[0] must be the identity exactly")
        fro = lambda x: x.flatten(-2).norm(dim=-1)
        if float(fro(S @ S.transpose(-1, -2) - eye).max()) > SYM_TOL or float((torch.linalg.det(S) - 1).abs().max()) > SYM_TOL:
            raise ValueError("every element must be a rotation")
        # closure: every product (and so, in a finite set of rotations holding the identity, every inverse) is an element
        P = S[:, :, None] @ S[:, None, :]                                           # (b,G,G,3,3)
        d = fro(P[:, :, :, None] - S[:, None, None, :])                            # (b,G,G,G)
        if float(d.min(dim=-1).values.max()) > SYM_TOL:
            raise ValueError("the set is not closed under product")
        dinv = fro(S.transpose(-1, -2)[:, :, None] - S[:, None, :])
        if float(dinv.min(dim=-1).values.max()) > SYM_TOL:
            raise ValueError("the set is not closed under inverse")
        if self.axis is not None:
            a = self.axis.detach().cpu().to(torch.float64).reshape(-1, 3)
            if float((a.norm(dim=-1) - 1).abs().max()) > SYM_TOL:
                raise ValueError("axis must be a unit vector")
            Sa = (S @ a[:, None, :, None])[..., 0]                                  # (b,G,3) (b broadcasts)
            e = torch.minimum((Sa - a[:, None]).norm(dim=-1), (Sa + a[:, None]).norm(dim=-1))
            if float(e.max()) > SYM_TOL:
                raise ValueError("every element must map the axis to +- itself")

    @property
    def order(self) -> int:
        return self.S.shape[-3]

    @property
    def trivial(self) -> bool:
        return self.order == 1 and self.axis is None

    @property
    def device(self):
        return self.S.device

    def to(self, device) -> "Symmetry":
        out = object.__new__(Symmetry)   # (already checked)
        out.S = self.S.to(device)
        out.axis = None if self.axis is None else self.axis.to(device)
        return out

    def conjugate(self, P) -> "Symmetry":
        """The group in another frame: ``P S P^T`` and ``P a`` for ``P (3,3)`` or ``(B,3,3)`` (fp64 products rounded to fp32;
        element 0 stays the identity exactly)."""
        P = torch.as_tensor(P).to(device=self.S.device, dtype=torch.float64)
        if tuple(P.shape) != (3, 3) and not (P.dim() == 3 and tuple(P.shape[1:]) == (3, 3)):
            raise ValueError("P must be (3,3) or (B,3,3), got %s" % (tuple(P.shape),))
        if P.dim() == 3 and self.S.dim() == 4 and P.shape[0] != self.S.shape[0]:
            raise ValueError("P and S disagree on B")
        S = self.S.to(torch.float64)
        Pb = P if P.dim() == 2 else P[:, None]
        if P.dim() == 3 and S.dim() == 3:
            S = S[None]
        C = (Pb @ S @ Pb.transpose(-1, -2)).to(torch.float32)
        C[..., 0, :, :] = torch.eye(3, dtype=torch.float32, device=C.device)
        axis = None
        if self.axis is not None:
            a = self.axis.to(torch.float64)
            axis = (P @ a[..., None])[..., 0]
            axis = (axis / axis.norm(dim=-1, keepdim=True)).to(torch.float32)
        return Symmetry(C, axis)

    # ---- constructors (fp64, rounded to fp32) ----
    @classmethod
    def _from_np(cls, S: np.ndarray, axis=None) -> "Symmetry":
        S = np.where(np.abs(S) < 1e-15, 0.0, S)   # exact zeros where the fp64 product left 1e-17
        return cls(torch.from_numpy(S.astype(np.float32)), None if axis is None else torch.from_numpy(axis.astype(np.float32)))

    @classmethod
    def trivial_group(cls) -> "Symmetry":
        return cls._from_np(np.eye(3)[None])

    @classmethod
    def cyclic(cls, n: int, axis="Z") -> "Symmetry":
        """C_n: the n rotations by multiples of 360 / n degrees about ``axis``."""
        a = _unit(axis)
        return cls._from_np(np.stack([_rot_np(a, 2.0 * math.pi * k / int(n)) for k in range(int(n))]))

    @classmethod
    def dihedral(cls, n: int, axis="Z") -> "Symmetry":
        """D_n (order 2n): C_n about ``axis`` and n half turns about axes perpendicular to it."""
        a = _unit(axis)
        flip = _rot_np(_perp(a), math.pi)
        rots = [_rot_np(a, 2.0 * math.pi * k / int(n)) for k in range(int(n))]
        return cls._from_np(np.stack(rots + [r @ flip for r in rots]))

    @classmethod
    def tetrahedral(cls) -> "Symmetry":
        """The 12 rotations of a regular tetrahedron (vertices on alternate cube corners)."""
        return cls._from_np(_closure([_rot_np(_unit((0, 0, 1)), math.pi), _rot_np(_unit((1, 1, 1)), 2.0 * math.pi / 3.0)]))

    @classmethod
    def octahedral(cls) -> "Symmetry":
        """The 24 rotations of the cube (signed permutation matrices of determinant 1: every entry 0 or +-1 exactly)."""
        return cls._from_np(np.round(_closure([_rot_np(_unit((0, 0, 1)), 0.5 * math.pi), _rot_np(_unit((1, 0, 0)), 0.5 * math.pi)])))

    @classmethod
    def icosahedral(cls) -> "Symmetry":
        """The 60 rotations of a regular icosahedron (a five-fold axis through (0, 1, phi), a three-fold one through (1, 1, 1))."""
        phi = 0.5 * (1.0 + math.sqrt(5.0))
        return cls._from_np(_closure([_rot_np(_unit((0, 1, phi)), 2.0 * math.pi / 5.0), _rot_np(_unit((1, 1, 1)), 2.0 * math.pi / 3.0)]))

    @classmethod
    def axial(cls, axis="Z", flip: bool = False) -> "Symmetry":
        """A solid of revolution about ``axis``: C_inf, or with ``flip`` D_inf (a half turn about a perpendicular axis as well)."""
        a = _unit(axis)
        S = [np.eye(3)] + ([_rot_np(_perp(a), math.pi)] if flip else [])
        return cls._from_np(np.stack(S), a)

    @classmethod
    def from_config(cls, entry) -> "Symmetry":
        """The reference's ``SYMMETRIC_OBJ`` entry: an axis letter and the symmetry angle in degrees -- ``['Z', 180]`` is
        ``cyclic(2, 'Z')``; an angle of 0 stands for a solid of revolution."""
        letter, angle = entry[0], float(entry[1])
        if angle == 0.0:
            return cls.axial(letter)
        n = 360.0 / angle
        if abs(n - round(n)) > 1e-9 or round(n) < 1:
            raise ValueError("symmetry angle %r does not divide 360 degrees" % (entry[1],))
        return cls.cyclic(int(round(n)), letter)


def _sym_trace(R_pred: torch.Tensor, R_gt: torch.Tensor, symmetry: Symmetry) -> torch.Tensor:
    """t_G(R_pred, R_gt) in plain torch, (n,): max over the group of sum (R_pred S) o R_gt."""
    Rp, Rg = R_pred.reshape(-1, 3, 3), R_gt.reshape(-1, 3, 3)
    S = symmetry.S.to(device=Rp.device, dtype=Rp.dtype)
    S = S[None] if S.dim() == 3 else S                                             # (1 | n, G, 3, 3)
    M = Rg.transpose(-1, -2)[:, None] @ Rp[:, None] @ S                             # A^T R S_g
    tr = M.diagonal(dim1=-2, dim2=-1).sum(-1)
    if symmetry.axis is None:
        return tr.max(dim=1).values
    a = symmetry.axis.to(device=Rp.device, dtype=Rp.dtype).reshape(-1, 1, 3)
    p = (a[..., None, :] @ M @ a[..., :, None])[..., 0, 0]
    c = tr - p
    s = -(a[..., 0] * (M[..., 2, 1] - M[..., 1, 2]) + a[..., 1] * (M[..., 0, 2] - M[..., 2, 0]) + a[..., 2] * (M[..., 1, 0] - M[..., 0, 1]))
    return (p + torch.sqrt(c * c + s * s)).max(dim=1).values


def geodesic_sym_deg(R_pred: torch.Tensor, R_gt: torch.Tensor, symmetry: Symmetry | None) -> torch.Tensor:
    """``geodesic_deg`` modulo a symmetry group: the smallest angular error over the poses equivalent to ``R_pred``,
    arccos((t_G.clamp(-1, 3) - 1) / 2) in degrees.  The metric, not a hot path: plain torch.  ``symmetry=None`` or the trivial
    group: ``geodesic_deg``."""
    if symmetry is None or symmetry.trivial:
        return geodesic_deg(R_pred, R_gt)
    sim = (_sym_trace(R_pred, R_gt, symmetry).clamp(-1, 3) - 1) / 2
    return torch.arccos(sim) * 180.0 / math.pi
