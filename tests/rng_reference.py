"""Host mirror of the device's random streams: Philox-4x32-10 -> Box-Muller -> Gaussian quaternion -> rotation, the two
compositions around it, and the (key, counter) tuple of every stream as ``include/ahv.h`` words it.  Plain numpy, written from
the algorithm's definition (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) and from the
header's text, not from the kernels.

Every float function takes ``dtype``:
  np.float64  the reference: the exact 24-bit uniforms, every later operation in fp64
  np.float32  the yardstick: the same operations, each rounded to fp32 (numpy keeps float32 arrays in float32)
The distance between the two on a case is e_ref, what fp32 costs there; a kernel is held to 4 e_ref (tests/oplevel_cases.py).

``source_constants`` / ``source_layouts`` read the tags, the fresh-slot seeds and the counter expressions out of ahv_so3.h,
ahv_track.hip and ahv_graph.hip, and ``c_eval`` evaluates such an expression with C's unsigned widths, so that the CPU twin
(tests/test_rng_cpu.py) can hold the sources to the header's layouts without a GPU.
"""
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "3dahv_amd", "csrc")
M32, M64 = (1 << 32) - 1, (1 << 64) - 1

# ---- what include/ahv.h states ------------------------------------------------------------------------------------------------
HAAR_TAG, DIFFUSE_TAG, VELOCITY_TAG, ADVANCE_TAG, GRAPH_TAG = 0x3D4148, 0x444946, 0x56454C, 0x414456, 0x504752
FRESH_XOR = 0x9E3779B97F4A7C15          # tracker and pose graph: fresh slots come from the Haar stream of seed ^ this

# ---- Philox-4x32-10 -----------------------------------------------------------------------------------------------------------
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57      # the two multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85      # the Weyl increments of the key: golden ratio, sqrt(3) - 1


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox4x32(c0, c1, c2, c3, k0, k1, rounds=10):
    """One block per element of the broadcast arguments -> four uint32 arrays.  A round maps (c0, c1, c2, c3) to
    (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key is bumped by (W0, W1) between rounds."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(x) for x in (c0, c1, c2, c3, k0, k1)))
    assert all(int(x.max(initial=0)) <= M32 for x in (c0, c1, c2, c3, k0, k1)), "32-bit words"
    lo = np.uint64(M32)
    s = np.uint64(32)
    for r in range(rounds):
        if r:
            k0, k1 = (k0 + np.uint64(PHILOX_W0)) & lo, (k1 + np.uint64(PHILOX_W1)) & lo
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2      # 32 x 32 bits: fits 64
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ k0, p1 & lo, (p0 >> s) ^ c3 ^ k1, p0 & lo
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    return philox4x32(c0, c1, c2, c3, k0, k1, 10)


def draw(block, rounds=10):
    """A stream's ``(k0, k1, c0, c1, c2, c3)`` -> the four output words."""
    k0, k1, c0, c1, c2, c3 = block
    return philox4x32(c0, c1, c2, c3, k0, k1, rounds)


# ---- words -> normals -> rotation ---------------------------------------------------------------------------------------------
TWO_PI = 6.28318530717958647692


def uniforms(words):
    """The four 24-bit uniforms of a block, exact in either format: u0, u2 in (0, 1] (they go into the log), u1, u3 in [0, 1)."""
    w = [np.asarray(x, dtype=np.uint32) >> np.uint32(8) for x in words]
    f = [x.astype(np.float64) for x in w]
    return (f[0] + 1.0) / 16777216.0, f[1] / 16777216.0, (f[2] + 1.0) / 16777216.0, f[3] / 16777216.0


def box_muller4(words, dtype=np.float64):
    """Two Box-Muller pairs: (g0, g1) from (u0, u1), (g2, g3) from (u2, u3); g = sqrt(-2 ln u_even) (cos, sin)(2 pi u_odd)."""
    u0, u1, u2, u3 = (x.astype(dtype) for x in uniforms(words))        # exact: 24-bit integers times 2^-24
    two, tau = dtype(2.0), dtype(TWO_PI)
    r0, r1 = np.sqrt(-two * np.log(u0)), np.sqrt(-two * np.log(u2))
    a0, a1 = tau * u1, tau * u3
    g = r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)
    assert all(x.dtype == dtype for x in g)
    return g


def quaternion_matrix(qr, qi, qj, qk, dtype=np.float64):
    """(qr, qi, qj, qk) of any norm > 0 -> (..., 3, 3)."""
    qr, qi, qj, qk = (np.asarray(x, dtype=dtype) for x in (qr, qi, qj, qk))
    one = dtype(1.0)
    t = dtype(2.0) / np.maximum(qr * qr + qi * qi + qj * qj + qk * qk, dtype(1e-30))
    o = np.stack([one - t * (qj * qj + qk * qk), t * (qi * qj - qk * qr), t * (qi * qk + qj * qr),
                  t * (qi * qj + qk * qr), one - t * (qi * qi + qk * qk), t * (qj * qk - qi * qr),
                  t * (qi * qk - qj * qr), t * (qj * qk + qi * qr), one - t * (qi * qi + qj * qj)], axis=-1)
    assert o.dtype == dtype
    return o.reshape(o.shape[:-1] + (3, 3))


def haar_quaternion(seed, ctr, dtype=np.float64):
    return box_muller4(draw(haar_block(seed, ctr)), dtype)


def haar_rotation(seed, ctr, dtype=np.float64):
    """Rotation ``ctr`` (array of Python ints or uint64) of the Haar stream of ``seed``."""
    return quaternion_matrix(*haar_quaternion(seed, ctr, dtype), dtype=dtype)


def shepperd_branch(R):
    """Which of the four divisions q(R) takes, per matrix: 0 trace > 0, else 1 / 2 / 3 for the largest diagonal entry."""
    R = np.asarray(R)
    r0, r4, r8 = R[..., 0, 0], R[..., 1, 1], R[..., 2, 2]
    return np.where(r0 + r4 + r8 > 0, 0, np.where((r0 > r4) & (r0 > r8), 1, np.where(r4 > r8, 2, 3)))


def rotation_quaternion(R, dtype=np.float64):
    """q(R) by Shepperd's branch: divide by the largest of the four components."""
    R = np.asarray(R, dtype=dtype)
    r = [R[..., a, c] for a in range(3) for c in range(3)]
    one, two, q4 = dtype(1.0), dtype(2.0), dtype(0.25)
    br = shepperd_branch(R)
    with np.errstate(invalid="ignore", divide="ignore"):        # the three branches not taken may see sqrt(< 0)
        s0 = two * np.sqrt(r[0] + r[4] + r[8] + one)
        s1 = two * np.sqrt(one + r[0] - r[4] - r[8])
        s2 = two * np.sqrt(one + r[4] - r[0] - r[8])
        s3 = two * np.sqrt(one + r[8] - r[0] - r[4])
        cand = [(q4 * s0, (r[7] - r[5]) / s0, (r[2] - r[6]) / s0, (r[3] - r[1]) / s0),
                ((r[7] - r[5]) / s1, q4 * s1, (r[1] + r[3]) / s1, (r[2] + r[6]) / s1),
                ((r[2] - r[6]) / s2, (r[1] + r[3]) / s2, q4 * s2, (r[5] + r[7]) / s2),
                ((r[3] - r[1]) / s3, (r[2] + r[6]) / s3, (r[5] + r[7]) / s3, q4 * s3)]
    return tuple(np.choose(br, [cand[k][m] for k in range(4)]).astype(dtype) for m in range(4))


def compose_rotation_vector(R, w, dtype=np.float64):
    """M(normalise(q(R) q(w))), the matrix of R exp([w]x): q(w) = (cos a/2, sin(a/2) w / a), a = |w|, with sin(a/2) / a taken
    as 1/2 - a^2/48 below a = 1e-3; the Hamilton product; one normalisation; quaternion_matrix.  R (..., 3, 3), w (..., 3)."""
    w = np.asarray(w, dtype=dtype)
    w0, w1, w2 = w[..., 0], w[..., 1], w[..., 2]
    a = np.sqrt(w0 * w0 + w1 * w1 + w2 * w2)
    half = dtype(0.5) * a
    with np.errstate(invalid="ignore", divide="ignore"):
        kq = np.where(a < dtype(1e-3), dtype(0.5) - a * a * dtype(1.0 / 48.0), np.sin(half) / a)
    dr, di, dj, dk = np.cos(half), kq * w0, kq * w1, kq * w2
    qr, qi, qj, qk = rotation_quaternion(R, dtype)
    pr = qr * dr - qi * di - qj * dj - qk * dk
    pi = qr * di + qi * dr + qj * dk - qk * dj
    pj = qr * dj - qi * dk + qj * dr + qk * di
    pk = qr * dk + qi * dj - qj * di + qk * dr
    inv = dtype(1.0) / np.sqrt(np.maximum(pr * pr + pi * pi + pj * pj + pk * pk, dtype(1e-30)))
    assert inv.dtype == dtype
    return quaternion_matrix(pr * inv, pi * inv, pj * inv, pk * inv, dtype)


CLIP_UP, CLIP_DOWN = float(np.float32(1.00000048)), float(np.float32(0.99999952))      # 1 + 2^-21, 1 - 2^-21


def clip_norm(w, limit, dtype=np.float64):
    """w (..., 3) scaled by (limit / |w|) (1 - 2^-21) where |w| (1 + 2^-21) > limit; limit 0: no limit.  -> (w', clipped)."""
    w = np.asarray(w, dtype=dtype)
    a = np.sqrt(w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1] + w[..., 2] * w[..., 2])
    limit = dtype(limit)
    if not limit > 0:
        return w, np.zeros(a.shape, dtype=bool)
    clipped = a * dtype(CLIP_UP) > limit
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(clipped, (limit / a) * dtype(CLIP_DOWN), dtype(1.0))
    out = w * s[..., None]
    assert out.dtype == dtype
    return out, clipped


def clip_distance(w, limit):
    """|w| (1 + 2^-21) / limit - 1 in fp64: how far, relatively, each slot sits from the clipping decision."""
    w = np.asarray(w, dtype=np.float64)
    return np.sqrt((w * w).sum(-1)) * CLIP_UP / float(limit) - 1.0


# ---- the streams: (k0, k1, c0, c1, c2, c3) as include/ahv.h words them ------------------------------------------------------------
def _ints(x):
    """Python ints of any size, as an object array: the layouts are integer arithmetic, done exactly."""
    return np.asarray(x, dtype=object)


def _words(*fields):
    out = np.broadcast_arrays(*(_ints(f) for f in fields))
    assert all(0 <= int(v) <= M32 for f in out for v in f.reshape(-1)), "a field left its 32-bit word"
    return tuple(f.astype(np.uint64) for f in out)


def _key(seed):
    seed = _ints(seed) & M64
    return seed & M32, seed >> 32              # key = seed: low word first


def haar_block(seed, ctr):
    """ahv_random_rotations_f32: rotation n of a call is block ctr = offset + n (modulo 2^64), third word 0x3D4148."""
    ctr = _ints(ctr) & M64
    return _words(*_key(seed), ctr & M32, ctr >> 32, HAAR_TAG, 0)


def _tracker_block(seed, step, b, j, tag):
    step = _ints(step)
    return _words(*_key(seed), _ints(j), _ints(b) | (((step >> 32) & 0xFFFF) << 16), tag, step & M32)


def diffuse_block(seed, step, b, j):
    """ahv_diffuse_rotations_f32: counter = (j, b | step[47:32] << 16, 0x444946, step[31:0])."""
    return _tracker_block(seed, step, b, j, DIFFUSE_TAG)


def velocity_block(seed, step, b, j):
    """ahv_predict_rotations_f32's second block: the diffusion block's counter with 0x56454C as its third word."""
    return _tracker_block(seed, step, b, j, VELOCITY_TAG)


def advance_block(seed, t1, b):
    """ahv_track_advance: u[b] of the step that becomes t1 = t + 1: counter = (b, t1[63:32], 0x414456, t1[31:0])."""
    t1 = _ints(t1) & M64
    return _words(*_key(seed), _ints(b), t1 >> 32, ADVANCE_TAG, t1 & M32)


def advance_u(seed, t1, b):
    """u[b] = (word 0 >> 8) 2^-24, exact in fp32."""
    return ((draw(advance_block(seed, t1, b))[0] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def tracker_fresh_offset(step, B, b, M, j):
    """(step B + b) M + j, step taken whole, modulo 2^64: the Haar block of seed ^ FRESH_XOR a fresh tracker slot holds."""
    return (((_ints(step) & M64) * B + _ints(b)) * M + _ints(j)) & M64


def graph_block(seed, t, sweep, b, k, n):
    """ahv_pose_graph_propose_f32: counter = (n, b | sweep << 16 | t[39:32] << 24, 0x504752 | k << 24, t[31:0])."""
    t = _ints(t)
    return _words(*_key(seed), _ints(n), _ints(b) | (_ints(sweep) << 16) | (((t >> 32) & 0xFF) << 24), GRAPH_TAG | (_ints(k) << 24),
                  t & M32)


def graph_fresh_offset(t, sweep, b, k, N, n):
    """(((t 256 + sweep) 65536 + b) 16 + k) N + n, modulo 2^64."""
    return ((((((_ints(t) & M64) * 256 + _ints(sweep)) * 65536 + _ints(b)) * 16 + _ints(k)) * N) + _ints(n)) & M64


def normals3(block, dtype=np.float64):
    """The first three normals of a block, (..., 3)."""
    g = box_muller4(draw(block), dtype)
    return np.stack(g[:3], axis=-1)


# ---- the sources --------------------------------------------------------------------------------------------------------------
def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def source_constants():
    """Tags and fresh-slot seeds as the three source files define them."""
    track, graph, so3 = _read("ahv_track.hip"), _read("ahv_graph.hip"), _read("ahv_so3.h")
    num = lambda name, text: int(re.search(r"\b%s\s*=\s*(0x[0-9A-Fa-f]+)u?(?:ll)?\s*[,;]" % name, text).group(1), 16)
    haar = re.search(r"unsigned c\[4\] = \{\(unsigned\)ctr, \(unsigned\)\(ctr >> 32\), (0x[0-9A-Fa-f]+)u, 0u\};", so3)
    return {"kHaarTag": int(haar.group(1), 16), "kDiffuseTag": num("kDiffuseTag", track), "kAdvanceTag": num("kAdvanceTag", track),
            "kVelocityTag": num("kVelocityTag", track), "kFreshSeed": num("kFreshSeed", track), "kGraphTag": num("kGraphTag", graph),
            "kGraphFreshSeed": num("kGraphFreshSeed", graph)}


def _body(text, signature):
    """The text of the function whose header contains ``signature``, from there to the closing brace in column 0."""
    start = text.index(signature)
    return text[start:text.index("\n}\n", start)]


def _braces(text):
    m = re.search(r"unsigned c\[4\] = \{(.*?)\};", text, flags=re.S)
    return [x.strip() for x in _split_top(m.group(1))]


def _split_top(s):
    parts, depth, cur = [], 0, ""
    for ch in s:
        depth += ch == "("
        depth -= ch == ")"
        if ch == "," and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    return parts + [cur]


def source_layouts():
    """The C expressions the kernels build their counters, keys and fresh offsets from, as text:
    {stream: {"counter": [four expressions]}} or {"offset": expression}, plus "keys": the key arguments of every Philox call."""
    track, graph, so3 = _read("ahv_track.hip"), _read("ahv_graph.hip"), _read("ahv_so3.h")
    diffuse, predict = _body(track, "void diffuse_slot("), _body(track, "void predict_slot(")
    advance, propose = _body(track, "void track_advance_kernel("), _body(graph, "void pose_graph_propose_kernel(")
    haar = _body(so3, "void haar_rotation(")
    fresh = lambda body: re.search(r"haar_rotation\(seed \^ (\w+), (.*), o\);", body).groups()
    cb = re.search(r"const unsigned cb = (.*?);", predict).group(1)
    second = re.search(r"c\[0\] = (.*?); c\[1\] = (.*?); c\[2\] = (.*?); c\[3\] = (.*?);", predict).groups()
    sub = lambda xs: ["(%s)" % cb if x == "cb" else x for x in xs]
    ctr = re.search(r"const unsigned long long ctr =\s*(.*?);", propose, flags=re.S).group(1)
    out = {"haar": {"counter": _braces(haar)},
           "diffuse": {"counter": _braces(diffuse)},
           "velocity": {"counter": sub(_braces(predict))},
           "predict_diffuse": {"counter": sub(list(second))},
           "advance": {"counter": _braces(advance), "t1": re.search(r"const unsigned long long t1 = (.*?);", advance).group(1)},
           "graph": {"counter": _braces(propose)},
           "tracker_fresh": {"offset": fresh(diffuse)[1], "xor": fresh(diffuse)[0]},
           "predict_fresh": {"offset": fresh(predict)[1], "xor": fresh(predict)[0]},
           "graph_fresh": {"offset": " ".join(ctr.split()),
                           "xor": re.search(r"haar_rotation\(seed \^ (\w+), ctr, q\);", propose).group(1)}}
    out["keys"] = [m for text in (track, graph, so3) for m in re.findall(r"philox4x32_10\(c, (.*?)\);", text)]
    return out


_TOKEN = re.compile(r"\s*(0x[0-9A-Fa-f]+|\d+|[A-Za-z_][\w.]*|<<|>>|[()*+\-|^&%])")
_BINARY = {"|": lambda a, b: a | b, "^": lambda a, b: a ^ b, "&": lambda a, b: a & b, "<<": lambda a, b: a << b,
           ">>": lambda a, b: a >> b, "+": lambda a, b: a + b, "-": lambda a, b: a - b, "*": lambda a, b: a * b,
           "%": lambda a, b: a % b}
_TYPES = {"unsigned": 32, "unsigned long long": 64, "long": 64, "long long": 64, "int": 32}


def c_eval(expr, env):
    """Value of a C integer expression of casts, literals, names and * % + - << >> & ^ |, with C's precedence and unsigned
    wrap-around at each operand's width: ``(unsigned)`` and the suffix ``u`` are 32 bits, ``(unsigned long long)``, ``(long)``
    and ``ull`` 64; a binary operation has the wider operand's width (a shift: its left operand's).  ``env``: name -> value
    or (value, bits); a bare value is 64 bits wide.  Signed operands are never negative here, so they are treated as unsigned."""
    toks, pos = [], 0
    expr = expr.strip()
    while pos < len(expr):
        m = _TOKEN.match(expr, pos)
        assert m, "cannot read %r at %d" % (expr, pos)
        tok, pos = m.group(1), m.end()
        if re.fullmatch(r"0x[0-9A-Fa-f]+|\d+", tok):          # a literal and its suffix
            suffix = re.match(r"(?i)ull|u|ll|l", expr[pos:])
            suffix = suffix.group(0).lower() if suffix else ""
            pos += len(suffix)
            toks.append(("num", (int(tok, 0), 64 if "l" in suffix else 32)))
        else:
            toks.append(("op" if not (tok[0].isalpha() or tok[0] == "_") else "name", tok))
    state = {"i": 0}

    def peek():
        return toks[state["i"]] if state["i"] < len(toks) else (None, None)

    def take():
        state["i"] += 1
        return toks[state["i"] - 1]

    def wrap(v, bits):
        return v & ((1 << bits) - 1), bits

    def cast_ahead():
        i = state["i"]
        if peek() != ("op", "("):
            return None
        words = []
        i += 1
        while i < len(toks) and toks[i][0] == "name" and toks[i][1] in ("unsigned", "long", "int"):
            words.append(toks[i][1])
            i += 1
        if words and i < len(toks) and toks[i] == ("op", ")"):
            state["i"] = i + 1
            return _TYPES[" ".join(words)]
        return None

    def unary():
        bits = cast_ahead()
        if bits is not None:
            return wrap(unary()[0], bits)
        kind, tok = take()
        if kind == "num":
            return tok
        if kind == "name":
            v = env[tok]
            return wrap(*v) if isinstance(v, tuple) else wrap(v, 64)
        assert tok == "(", tok
        v = level(0)
        assert take() == ("op", ")")
        return v

    LEVELS = [("|",), ("^",), ("&",), ("<<", ">>"), ("+", "-"), ("*", "%")]

    def level(n):
        if n == len(LEVELS):
            return unary()
        a, abits = level(n + 1)
        while peek()[0] == "op" and peek()[1] in LEVELS[n]:
            op = take()[1]
            b, bbits = level(n + 1)
            bits = abits if op in ("<<", ">>") else max(abits, bbits)
            a = _BINARY[op](a, b)
            a, abits = wrap(a, bits)
        return a, abits

    v = level(0)
    assert state["i"] == len(toks), "trailing text in %r" % expr
    return v[0]
