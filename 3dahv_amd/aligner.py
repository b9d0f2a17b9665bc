"""Host-side mirror of the reference's ``Feature_Aligner`` (modules/modules.py:49-124).

Same constructor, method names, argument meaning and -- attribute for attribute -- the same
``state_dict`` keys, so a Lightning ``.ckpt`` of the reference loads
with ``load_state_dict``.

* ``forward_3d2d`` (per hypothesis, hot) runs the HIP kernel through the C ABI.
* ``forward_2d3d`` (once per pair: conv embedding, sin/cos position code, the
  bidirectional 3D-aware transformer of transformer/attention.py:196-396, 3-D res-block) runs as ONE
  C-ABI call (``ahv_forward_2d3d_f32``, csrc/ahv_encoder.hip and its ahv_enc_*.h) for inference calls on the GPU at the
  reference's configuration (768 -> 256, 4 heads); training-style calls (autograd recording) and other widths
  (the ``encoder_small`` fixture) use stock torch operators.  Pinned to the reference by the ``encoder_small``
  (shrunken) and ``encoder_full`` (768/256/4x64/depth 4) golden fixtures.
"""
from __future__ import annotations

import math
import itertools
import operator
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops


# packed weight tables for the C ABI, kept outside the modules so that they are neither pickled nor deep-copied
_PACKED = weakref.WeakKeyDictionary()


# ----------------------------------------------------------------------------- weight packing for the C ABI
# These work on ANY module tree with the reference's attribute names (this file's mirror or the reference's
# own Feature_Aligner / BidirectionTransformer), which is what lets patch.install() rebind forward_2d3d.
#
# A packed table mixes ALIASES of live parameters (already contiguous fp32: biases, LayerNorm, w_out, w_ff*) with
# COPIES (q|k|v concatenation, tap-major conv weights, zero-padded 3-D conv weights).  In-place parameter updates
# (optimizer.step(), harness.fit, GraphedTrainStep) change the aliases but not the copies, so every table carries
# the version key of the parameters it was built from and is refreshed when that key differs: copies are
# re-filled IN PLACE (their addresses -- which a captured hipGraph has baked in -- stay valid); only when a
# parameter's storage itself moved does the table get new pointers (``moved``; graph owners then re-capture).
def _f32(t, device):
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


_get_version = operator.attrgetter("_version")


class _ParamList(list):
    """The parameters of a module, cached when its table is packed, plus the modules that own them: a parameter that
    is RE-REGISTERED as a new object (``mod.weight = nn.Parameter(...)``, parametrize / weight_norm, ``to_empty``) leaves
    the old object's version counter and address untouched, so the key also carries the identities found in the owners'
    ``_parameters`` dicts right now."""
    __slots__ = ("owners",)


def _param_list(module):
    pl = _ParamList(module.parameters())
    pl.owners = [m._parameters for m in module.modules() if m._parameters]
    return pl


def _version_key(params):
    """(in-place update counters, storage addresses, identities of the registered parameter objects) of a CACHED
    parameter list: C-level map passes, ~40 us for the aligner's 229 parameters.  Walking ``module.parameters()`` on
    every call (round 2) cost ~350 us of Python per forward_2d3d -- more than the 0.3 ms of GPU work it guards.  The
    list is taken when the table is packed; ``load_state_dict`` and ``invalidate_packed`` drop the table (and the
    list with it); a changed key re-walks the module (``_Packed.refresh``)."""
    ids = tuple(map(id, itertools.chain.from_iterable(map(dict.values, params.owners))))
    return tuple(map(_get_version, params)), tuple(map(torch.Tensor.data_ptr, params)), ids


class _Packed:
    __slots__ = ("table", "keep", "device", "key", "entries", "epoch", "params")

    def __init__(self, table, device):
        self.table, self.device = table, device
        self.keep, self.entries, self.key, self.epoch, self.params = [], [], None, 0, []

    def put(self, setter, build):
        """setter(ptr) stores the device pointer in the C struct; build() returns the fp32 tensor."""
        t = build()
        self.keep.append(t)
        self.entries.append((setter, build))
        setter(t.data_ptr())

    def refresh(self, module):
        """Re-evaluate every entry after a parameter change; returns True when any pointer changed."""
        self.params = _param_list(module)  # a changed key may also mean re-registered parameters: re-walk once
        live = {p.untyped_storage().data_ptr() for p in self.params}
        moved = False
        for i, (setter, build) in enumerate(self.entries):
            new, old = build(), self.keep[i]
            if new.data_ptr() == old.data_ptr():
                continue  # alias of a live parameter (or a constant): already current
            if new.untyped_storage().data_ptr() not in live and new.shape == old.shape:
                old.copy_(new)  # a derived copy: refill in place, address unchanged
            else:  # an alias whose parameter storage itself moved (.to(), .data = ...)
                self.keep[i] = new
                setter(new.data_ptr())
                moved = True
        if moved:
            self.epoch += 1
        return moved


def _entry(param_fn, device):
    """build() for one packed tensor: param_fn() gives the (possibly derived) tensor from the live parameters."""
    return lambda: _f32(param_fn(), device)


def _struct_setter(struct, name, index=None):
    def set_(ptr):
        if index is None:
            setattr(struct, name, ptr)
        else:
            getattr(struct, name)[index] = ptr
    return set_


def pack_transformer(att, device):
    """ahv_block_weights table: per layer attn_self_1, attn_self_2, attn_cross_1, attn_cross_2; q|k|v weights
    concatenated to one [768][256] matrix (one GEMM for self-attention, row slices for cross-attention)."""
    from . import _lib
    table = (_lib.BlockWeights * (4 * len(att.transformer_blocks)))()
    pk = _Packed(table, device)
    i = 0
    for layer in att.transformer_blocks:
        for blk in (layer.attn_self_1, layer.attn_self_2, layer.attn_cross_1, layer.attn_cross_2):
            a, ff = blk.attn, blk.ff
            fns = dict(
                w_qkv=lambda a=a: torch.cat([a.to_q.weight, a.to_k.weight, a.to_v.weight], dim=0),
                w_out=lambda a=a: a.to_out[0].weight, b_out=lambda a=a: a.to_out[0].bias,
                ln1_g=lambda b=blk: b.norm1.weight, ln1_b=lambda b=blk: b.norm1.bias,
                w_ff1=lambda f=ff: f.net[0].proj.weight, b_ff1=lambda f=ff: f.net[0].proj.bias,
                w_ff2=lambda f=ff: f.net[2].weight, b_ff2=lambda f=ff: f.net[2].bias,
                ln2_g=lambda b=blk: b.norm2.weight, ln2_b=lambda b=blk: b.norm2.bias)
            for name, fn in fns.items():
                pk.put(_struct_setter(table[i], name), _entry(fn, device))
            i += 1
    pk.params = _param_list(att)
    pk.key = _version_key(pk.params)
    _PACKED[att] = pk
    return pk


def posemb_sincos_2d_tokens(channel: int, device, temperature: float = 10000.0) -> torch.Tensor:
    """modules/modules.py:72-84 evaluated on the 8x8 grid, token-major [h*8+w][channel]."""
    n = channel // 4
    omega = 1.0 / (temperature ** (torch.arange(n, device=device) / (n - 1)))
    ys, xs = torch.meshgrid(torch.arange(8, device=device), torch.arange(8, device=device), indexing="ij")
    ay, ax = ys[None] * omega[:, None, None], xs[None] * omega[:, None, None]
    pe = torch.cat((ax.sin(), ax.cos(), ay.sin(), ay.cos()), dim=0).type(torch.float32)
    return pe.reshape(channel, 64).t().contiguous()


def _packed_transformer(att, device):
    """Current table of `att` on `device` (built, refreshed or reused according to the version key)."""
    pk = _PACKED.get(att)
    if pk is None or pk.device != device:
        return pack_transformer(att, device)
    if _version_key(pk.params) != pk.key:
        pk.refresh(att)
        pk.key = _version_key(pk.params)
    return pk


def pack_aligner(fa, device):
    """ahv_aligner_weights (include/ahv.h): conv weights repacked tap-major, the 1x1x1 skip of the 3-D
    res-block folded into its first convolution as 16 extra output rows."""
    from . import _lib
    blocks = _packed_transformer(fa.att, device)
    rb2, rb3 = fa.feature_embedding[1], fa.feature_embedding_3d

    def w3d_1():
        w = torch.zeros(32, 32, 32, dtype=torch.float32, device=rb3.conv1.weight.device)  # [row][tap padded to 32][ci]
        w[:16, :27] = rb3.conv1.weight.detach().permute(0, 2, 3, 4, 1).reshape(16, 27, 32)
        w[16:, 13] = rb3.downsample[0].weight.detach().reshape(16, 32)  # centre tap (1,1,1) = 1*9 + 1*3 + 1
        return w.reshape(32, 1024)

    def w3d_2():
        w = torch.zeros(16, 32, 16, dtype=torch.float32, device=rb3.conv2.weight.device)
        w[:, :27] = rb3.conv2.weight.detach().permute(0, 2, 3, 4, 1).reshape(16, 27, 16)
        return w.reshape(16, 512)

    posemb = posemb_sincos_2d_tokens(256, device)  # a constant, not a parameter
    fns = dict(
        w_emb=lambda: fa.feature_embedding[0].weight.reshape(256, 768),
        w_conv1=lambda: rb2.conv1.weight.permute(0, 2, 3, 1).reshape(256, 2304),
        w_conv2=lambda: rb2.conv2.weight.permute(0, 2, 3, 1).reshape(256, 2304),
        posemb=lambda: posemb, gn_g=lambda: fa.att.norm.weight, gn_b=lambda: fa.att.norm.bias,
        w3d_1=w3d_1, w3d_2=w3d_2)
    pairs = dict(
        w_in=(lambda: fa.att.proj_in.weight.reshape(256, 256), lambda: fa.att.proj_context_in.weight.reshape(256, 256)),
        b_in=(lambda: fa.att.proj_in.bias, lambda: fa.att.proj_context_in.bias),
        w_out=(lambda: fa.att.proj_out.weight.reshape(256, 256), lambda: fa.att.proj_context_out.weight.reshape(256, 256)),
        b_out=(lambda: fa.att.proj_out.bias, lambda: fa.att.proj_context_out.bias))
    aw = _lib.AlignerWeights()
    pk = _Packed(aw, device)
    for name, fn in fns.items():
        pk.put(_struct_setter(aw, name), _entry(fn, device))
    for name, (fa_, fb_) in pairs.items():
        pk.put(_struct_setter(aw, name, 0), _entry(fa_, device))
        pk.put(_struct_setter(aw, name, 1), _entry(fb_, device))
    aw.blocks, aw.depth = blocks.table, len(fa.att.transformer_blocks)
    pk.keep.append(blocks)  # keeps the block table (and its tensors) alive with this one
    pk.params = _param_list(fa)
    pk.key = _version_key(pk.params)
    _PACKED[fa] = pk
    return pk


def _packed_aligner(fa, device):
    pk = _PACKED.get(fa)
    if pk is None or pk.device != device or _PACKED.get(fa.att) is not pk.keep[-1]:
        return pack_aligner(fa, device)
    if _version_key(pk.params) != pk.key:  # fa's list contains fa.att's parameters: one check covers both tables
        _packed_transformer(fa.att, device)  # refresh the block table first
        pk.refresh(fa)
        pk.key = _version_key(pk.params)
    return pk


def packed_epoch(fa) -> int:
    """Changes whenever a packed POINTER of `fa` changed (graph owners compare it and re-capture)."""
    pk, pa = _PACKED.get(fa), _PACKED.get(getattr(fa, "att", None)) if hasattr(fa, "att") else None
    return (pk.epoch if pk is not None else -1, pa.epoch if pa is not None else -1, id(pk), id(pa))


@torch.no_grad()
def hip_forward_2d3d(fa, src, tgt):
    """forward_2d3d(random_mask=False) of `fa` (mirror or reference module) through ahv_forward_2d3d_f32."""
    import ctypes
    from . import _lib
    packed = _packed_aligner(fa, src.device)
    B = src.shape[0]
    lib = _lib.load()
    nbytes = lib.ahv_forward_2d3d_workspace_bytes(B)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=src.device)
    vol_src = torch.empty((B, 16, 8, 8, 8), dtype=torch.float32, device=src.device)
    vol_tgt = torch.empty_like(vol_src)
    # keep the contiguous copies alive until the launch is enqueued: a temporary whose data_ptr() is taken inline is
    # returned to the allocator at once and the NEXT temporary may land on the same block (strided batches, e.g. the
    # harness's feats[:, 0], then read the target's copy as the source)
    src_c, tgt_c = src.detach().contiguous(), tgt.detach().contiguous()
    with torch.cuda.device(src.device):  # the C side sizes grids from the current device; launch on ITS stream
        _lib.check(lib.ahv_forward_2d3d_f32(ctypes.byref(packed.table), src_c.data_ptr(),
                                            tgt_c.data_ptr(), B, ws.data_ptr(), nbytes,
                                            vol_src.data_ptr(), vol_tgt.data_ptr(),
                                            torch.cuda.current_stream(src.device).cuda_stream), "ahv_forward_2d3d_f32")
    return vol_src, vol_tgt


def invalidate_packed(module):
    """Forget the packed weight tables of `module` (after its parameters changed)."""
    _PACKED.pop(module, None)
    att = getattr(module, "att", None)
    if att is not None:
        _PACKED.pop(att, None)


# ----------------------------------------------------------------------------- encoder pieces
class _GatedProj(nn.Module):
    """GEGLU input projection (transformer/attention.py:81-88): Linear -> (x, gate) -> x * gelu(gate)."""

    def __init__(self, dim_in: int, dim_out: int):
        super().__init__()
        self.proj = nn.Linear(dim_in, 2 * dim_out)

    def forward(self, t):
        val, gate = self.proj(t).chunk(2, dim=-1)
        return val * F.gelu(gate)  # exact erf GELU, as in the reference


class _FF(nn.Module):
    """FeedForward(2*dim -> dim, mult 4, gated) (transformer/attention.py:91-108); keys net.0.proj.*, net.2.*"""

    def __init__(self, dim_in: int, dim_out: int, mult: int = 4):
        super().__init__()
        inner = int(dim_in * mult)
        self.net = nn.ModuleList([_GatedProj(dim_in, inner), nn.Identity(), nn.Linear(inner, dim_out)])

    def forward(self, t):
        return self.net[2](self.net[0](t))


class _Attention(nn.Module):
    """Multi-head attention, q/k/v without bias, output projection with bias
    (transformer/attention.py:196-237); keys to_q/to_k/to_v.weight, to_out.0.{weight,bias}."""

    def __init__(self, dim: int, heads: int, dim_head: int):
        super().__init__()
        inner = heads * dim_head
        self.heads, self.scale = heads, dim_head ** -0.5
        self.to_q = nn.Linear(dim, inner, bias=False)
        self.to_k = nn.Linear(dim, inner, bias=False)
        self.to_v = nn.Linear(dim, inner, bias=False)
        self.to_out = nn.ModuleList([nn.Linear(inner, dim)])

    def forward(self, x, ctx):
        B, n, _ = x.shape
        split = lambda t: t.reshape(B, t.shape[1], self.heads, -1).transpose(1, 2)  # (B,h,n,d)
        q, k, v = split(self.to_q(x)), split(self.to_k(ctx)), split(self.to_v(ctx))
        att = torch.softmax((q @ k.transpose(-1, -2)) * self.scale, dim=-1)
        out = (att @ v).transpose(1, 2).reshape(B, n, -1)
        return self.to_out[0](out)


class _Block(nn.Module):
    """BasicTransformerBlock (transformer/attention.py:240-258):
    m = LN1(attn(x, ctx)); m = LN2(FF(cat[x, m])); return x + m."""

    def __init__(self, dim: int, heads: int, dim_head: int):
        super().__init__()
        self.attn = _Attention(dim, heads, dim_head)
        self.ff = _FF(2 * dim, dim)
        self.norm1 = nn.LayerNorm(dim)
        self.norm2 = nn.LayerNorm(dim)

    def forward(self, x, ctx=None):
        m = self.norm1(self.attn(x, x if ctx is None else ctx))
        m = self.norm2(self.ff(torch.cat([x, m], dim=2)))
        return x + m


class _BiBlock(nn.Module):
    """BidirectionTransformerBlock (transformer/attention.py:260-274): self(src), self(tgt),
    cross(src<-tgt), cross(tgt<-src), the two crosses reading the SAME post-self tensors."""

    def __init__(self, dim: int, heads: int, dim_head: int):
        super().__init__()
        self.attn_self_1 = _Block(dim, heads, dim_head)
        self.attn_self_2 = _Block(dim, heads, dim_head)
        self.attn_cross_1 = _Block(dim, heads, dim_head)
        self.attn_cross_2 = _Block(dim, heads, dim_head)

    def forward(self, x, ctx):
        x, ctx = self.attn_self_1(x), self.attn_self_2(ctx)
        return self.attn_cross_1(x, ctx), self.attn_cross_2(ctx, x)


class BidirectionTransformer(nn.Module):
    """The reference's "3D-aware encoder" (transformer/attention.py:336-396): ONE shared GroupNorm
    (32 groups, eps 1e-6), separate 1x1 in/out projections per stream, `depth` bidirectional blocks
    over 64 tokens, residual to the un-normalised inputs."""

    def __init__(self, in_channels: int, n_heads: int, d_head: int, depth: int = 1, dropout: float = 0.0,
                 context_dim=None, normalize: bool = True):
        super().__init__()
        if dropout != 0.0 or not normalize:
            raise NotImplementedError("the reference always uses dropout=0 and normalize=True")
        inner = n_heads * d_head
        self.norm = nn.GroupNorm(32, in_channels, eps=1e-6, affine=True)
        self.proj_in = nn.Conv2d(in_channels, inner, 1)
        self.proj_context_in = nn.Conv2d(in_channels if context_dim is None else context_dim, inner, 1)
        self.transformer_blocks = nn.ModuleList([_BiBlock(inner, n_heads, d_head) for _ in range(depth)])
        self.proj_out = nn.Conv2d(inner, in_channels, 1)
        self.proj_context_out = nn.Conv2d(inner, in_channels, 1)

        self.inner_dim, self.n_heads, self.d_head = inner, n_heads, d_head
        self.use_hip = True  # token stage on the HIP kernels when the tensors are on the GPU
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.invalidate_packed())

    # ---- HIP token stage (csrc/ahv_encoder.hip, kernels in ahv_enc_*.h) -------------------------------------------------
    def invalidate_packed(self):
        """Drop the packed weight table (call after changing parameters in place)."""
        _PACKED.pop(self, None)

    def _hip_eligible(self, xs):
        return (self.use_hip and xs.is_cuda and xs.dtype == torch.float32 and self.inner_dim == 256
                and self.n_heads == 4 and self.d_head == 64 and xs.shape[1] == 64 and not torch.is_grad_enabled())

    def _pack(self, device):
        return _packed_transformer(self, device)

    def _hip_blocks(self, xs, cs):
        from . import _lib
        table = _packed_transformer(self, xs.device).table
        B = xs.shape[0]
        xs, cs = xs.contiguous().clone(), cs.contiguous().clone()  # the kernels update the streams in place
        lib = _lib.load()
        nbytes = lib.ahv_transformer_workspace_bytes(B)
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=xs.device)
        with torch.cuda.device(xs.device):
            _lib.check(lib.ahv_transformer_blocks_f32(table, len(self.transformer_blocks), xs.data_ptr(), cs.data_ptr(),
                                                      B, ws.data_ptr(), nbytes,
                                                      torch.cuda.current_stream(xs.device).cuda_stream),
                       "ahv_transformer_blocks_f32")
        return xs, cs

    def forward(self, x, context):
        b, _, h, w = x.shape
        tok = lambda t: t.flatten(2).transpose(1, 2)                      # (B, hw, C)
        img = lambda t, hh, ww: t.transpose(1, 2).reshape(b, -1, hh, ww)  # back to (B, C, h, w)
        xs = tok(conv_mm(self.proj_in, self.norm(x)))
        cs = tok(conv_mm(self.proj_context_in, self.norm(context)))
        if self._hip_eligible(xs):
            xs, cs = self._hip_blocks(xs, cs)
        else:  # other widths (test fixtures), autograd, CPU tensors: stock torch operators
            for blk in self.transformer_blocks:
                xs, cs = blk(xs, cs)
        hc, wc = context.shape[-2:]
        return (conv_mm(self.proj_out, img(xs, h, w)) + x,
                conv_mm(self.proj_context_out, img(cs, hc, wc)) + context)


def conv_mm(conv: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """``conv(x)`` for the 1x1 / 3x3(x3) stride-1 same-padding convolutions of the aligner, evaluated as
    unfold + matmul when autograd is recording on the GPU.  Same arithmetic, different operator: MIOpen has no
    tuned fp32 kernels for these tiny 8x8 / 8^3 images on gfx950 and falls back to ``naive_conv_*`` -- 12 ms of a
    23-ms encoder forward+backward at B = 12 (rocprofv3) -- whereas the GEMM form goes through hipBLASLt/rocBLAS in
    both directions.  Everywhere else (CPU, no_grad) the convolution module itself runs."""
    if not (x.is_cuda and torch.is_grad_enabled()):
        return conv(x)
    return conv_as_matmul(conv, x)


def conv_as_matmul(conv: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """The GEMM form behind ``conv_mm``: kernel 1 or 3, stride 1, padding k // 2, 2-D or 3-D."""
    w, k = conv.weight, conv.kernel_size[0]
    B, C = x.shape[:2]
    sp = x.shape[2:]
    if k == 1:
        out = w.reshape(w.shape[0], C) @ x.flatten(2)
    elif x.dim() == 4:
        out = w.reshape(w.shape[0], -1) @ F.unfold(x, 3, padding=1)
    else:
        cols = F.pad(x, (1, 1, 1, 1, 1, 1)).unfold(2, 3, 1).unfold(3, 3, 1).unfold(4, 3, 1)  # (B,C,D,H,W,3,3,3)
        cols = cols.permute(0, 1, 5, 6, 7, 2, 3, 4).reshape(B, C * 27, -1)
        out = w.reshape(w.shape[0], -1) @ cols
    out = out.reshape(B, -1, *sp)
    if conv.bias is not None:
        out = out + conv.bias.reshape(1, -1, *([1] * len(sp)))
    return out


class _ResBlock(nn.Module):
    """ResNetBlock_2D / _3D with BN=False (modules/modules.py:9-47,126-164): conv-relu-conv + skip
    (1x1 conv skip when channels change).  ``bn_down`` exists in the reference's state dict but is
    never applied in its forward (modules/modules.py:28-30 vs :32-47); kept for key parity only."""

    def __init__(self, cin: int, cout: int, three_d: bool):
        super().__init__()
        conv = nn.Conv3d if three_d else nn.Conv2d
        self.conv1 = conv(cin, cout, 3, padding=1, bias=False)
        self.conv2 = conv(cout, cout, 3, padding=1, bias=False)
        self.downsample = None
        if cin != cout:
            self.downsample = nn.Sequential(conv(cin, cout, 1, bias=False))
            self.bn_down = (nn.BatchNorm3d if three_d else nn.BatchNorm2d)(cout)

    def forward(self, x):
        out = conv_mm(self.conv2, F.relu(conv_mm(self.conv1, x)))
        return out + (x if self.downsample is None else conv_mm(self.downsample[0], x))


def random_masking(x: torch.Tensor, mask_ratio: float) -> torch.Tensor:
    """Train-time voxel masking (utils.py:133-158): keep a random (1-ratio) subset of the L=D*H*W
    sites per sample; with probability 1/2 a sample is left unmasked.  Returns (N, L) float mask."""
    N, L = x.shape[0], x[0, 0].numel()
    keep = int(L * (1 - mask_ratio))
    order = torch.argsort(torch.rand(N, L, device=x.device), dim=1)
    gate = torch.rand(N, device=x.device) > 0.5
    ranked = torch.zeros(N, L, device=x.device)
    ranked[:, :keep] = 1
    mask = torch.gather(ranked, 1, order)
    return ((mask + gate[:, None].float()) > 0).float()


# ----------------------------------------------------------------------------- the aligner
class Feature_Aligner(nn.Module):
    """Drop-in for the reference class of the same name (modules/modules.py:49-124)."""

    def __init__(self, in_channel: int = 256, mid_channel: int = 256, out_channel: int = 32, n_heads: int = 4,
                 depth: int = 4):
        super().__init__()
        self.in_channel, self.mid_channel, self.out_channel = in_channel, mid_channel, out_channel
        self.feature_embedding = nn.Sequential(nn.Conv2d(in_channel, mid_channel, 1, bias=False),
                                               _ResBlock(mid_channel, mid_channel, three_d=False))
        self.att = BidirectionTransformer(mid_channel, n_heads=n_heads, d_head=mid_channel // n_heads, depth=depth,
                                          dropout=0.0, context_dim=mid_channel, normalize=True)
        self.feature_embedding_3d = _ResBlock(mid_channel // 8, 16, three_d=True)
        self.feature_embedding_2d = nn.Sequential(nn.Conv2d(3 * 8 * 16, out_channel, 1, bias=False),
                                                  nn.ReLU(inplace=True), nn.Conv2d(out_channel, out_channel, 1))
        self.use_hip_encoder = True  # forward_2d3d on the HIP kernels when the inputs are on the GPU
        self.register_load_state_dict_post_hook(lambda module, incompatible: _PACKED.pop(module, None))

    def posemb_sincos_2d(self, patches, channel=128, temperature=10000, dtype=torch.float32):
        """cat(sin x, cos x, sin y, cos y) with channel/4 frequencies 1/T^(k/(channel/4-1))
        (modules/modules.py:72-84); returns (channel, h, w)."""
        h, w = patches.shape[-2:]
        assert channel % 4 == 0, "feature dimension must be multiple of 4 for sincos emb"
        n = channel // 4
        omega = 1.0 / (temperature ** (torch.arange(n, device=patches.device) / (n - 1)))
        ys, xs = torch.meshgrid(torch.arange(h, device=patches.device), torch.arange(w, device=patches.device),
                                indexing="ij")
        ay, ax = ys[None] * omega[:, None, None], xs[None] * omega[:, None, None]
        return torch.cat((ax.sin(), ax.cos(), ay.sin(), ay.cos()), dim=0).type(dtype)

    # ---- whole forward_2d3d on the HIP kernels (csrc/ahv_encoder.hip, ahv_enc_*.h) -----------------------------
    def _hip_2d3d_eligible(self, x):
        return (self.use_hip_encoder and x.is_cuda and x.dtype == torch.float32 and self.in_channel == 768
                and self.mid_channel == 256 and tuple(x.shape[1:]) == (768, 8, 8) and self.att.n_heads == 4
                and self._inference_call())

    def _inference_call(self) -> bool:
        """no_grad, or a module in eval mode: the reference's evaluation scripts only call ``model.eval()``
        (test_co3d.py:219) and leave grad mode on, so eval mode is what marks inference.  The HIP encoder has no
        autograd edge: such a call returns detached volumes.  A module in training mode with autograd recording
        runs the stock-torch operators below (differentiable), as does any other width or a CPU tensor."""
        return (not torch.is_grad_enabled()) or (not self.training)

    def _pack_aligner(self, device):
        return _packed_aligner(self, device)

    def _hip_forward_2d3d(self, src, tgt):
        return hip_forward_2d3d(self, src, tgt)

    def forward_2d3d(self, img_feat_src, img_feat_tgt, random_mask=True, mask_ratio=0.25):
        """(B,in,8,8) x2 -> (B,16,8,8,8) x2 (modules/modules.py:86-110)."""
        bs = img_feat_src.shape[0]
        if self._hip_2d3d_eligible(img_feat_src):
            src, tgt = self._hip_forward_2d3d(img_feat_src, img_feat_tgt)
            if random_mask is True:
                src = src * random_masking(src, mask_ratio).reshape(-1, 1, 8, 8, 8)
                tgt = tgt * random_masking(tgt, mask_ratio).reshape(-1, 1, 8, 8, 8)
            return src, tgt
        embed = lambda t: self.feature_embedding[1](conv_mm(self.feature_embedding[0], t))
        src, tgt = embed(img_feat_src), embed(img_feat_tgt)
        pe = self.posemb_sincos_2d(src, channel=self.mid_channel)[None]
        src, tgt = self.att(src + pe, tgt + pe)
        # channel index = c' * 8 + d: the 2-D map's channels become (c', depth)
        src = self.feature_embedding_3d(src.reshape(bs, self.mid_channel // 8, 8, 8, 8))
        tgt = self.feature_embedding_3d(tgt.reshape(bs, self.mid_channel // 8, 8, 8, 8))
        if random_mask is True:
            src = src * random_masking(src, mask_ratio).reshape(-1, 1, 8, 8, 8)
            tgt = tgt * random_masking(tgt, mask_ratio).reshape(-1, 1, 8, 8, 8)
        return src, tgt

    def head_weights(self):
        """(W1 (32,384), W2 (32,32), b2 (32,)) views of feature_embedding_2d for the C ABI."""
        c1, c2 = self.feature_embedding_2d[0], self.feature_embedding_2d[2]
        return c1.weight.reshape(c1.out_channels, -1), c2.weight.reshape(c2.out_channels, -1), c2.bias

    def forward_3d2d(self, img_feat):
        """(M,16,8,8,8) -> (M,32,64), unit norm over dim 1 (modules/modules.py:112-124). HIP kernel."""
        if self.out_channel != 32:
            raise NotImplementedError("the HIP head is built for out_channel=32 (the reference's only value)")
        W1, W2, b2 = self.head_weights()
        return ops.forward_3d2d(img_feat, W1, W2, b2)  # carries an autograd edge (HIP backward) when one is needed

    def verify_hypotheses(self, img_feat_src, img_feat_tgt, proposals, want_scores=False, topk=None, **kw):
        """test_co3d.py:137-145 as ONE launch with this module's head weights -> (scores | None, packed keys); an inference call
        by the rule of ``_inference_call`` (no_grad, or eval mode).  Same method ``patch.install()`` gives the reference's class.
        ``topk=K``: a third element, the K best hypotheses as packed keys (B,K) (``ops.select_topk`` decodes them)."""
        from .patch import verify_hypotheses
        return verify_hypotheses(self, img_feat_src, img_feat_tgt, proposals, want_scores=want_scores, topk=topk, **kw)

    def verify_views(self, vol_refs, vol_query, hypotheses, view_poses, **kw):
        """The verify step against V posed reference views with this module's head weights (``ops.verify_views``):
        ``vol_refs (B,V,16,8,8,8)`` with absolute rotations ``view_poses (B,V,3,3)``, the query volume ``(B,16,8,8,8)`` and
        ``hypotheses`` of the query's absolute rotation -> ``(fused scores (B,N) | None, packed keys)``;
        ``ops.select_rotation(keys, hypotheses)`` decodes the pose.  Keywords go to ``ops.verify_views``: with
        ``max_view_angle_deg``, ``compact=True`` (and ``capacity`` / ``want_counts``) scores only the pairs the limit lets take
        part, to the same bits.  An inference call by the rule of ``verify_hypotheses`` (no_grad, or eval mode); a module in
        training mode with autograd recording is refused."""
        from .patch import _inference_call
        if not _inference_call(self):
            raise RuntimeError("verify_views is the inference step (no autograd edge); the module is in training mode with "
                               "autograd recording -- use rotate_volume / forward_3d2d (differentiable) or "
                               "ops.score_hypotheses_autograd for the loss")
        W1, W2, b2 = self.head_weights()
        with torch.no_grad():
            return ops.verify_views(vol_refs.detach(), vol_query.detach(), hypotheses, view_poses, W1, W2, b2, **kw)

    # ---- once-per-pair encoder replayed from a hipGraph -------------------------------------------
    def graphed_forward_2d3d(self, batch: int = 1):
        """Returns ``fn(layer4_src, layer4_tgt) -> (vol_src, vol_tgt)`` that replays ``forward_2d3d``
        (inference form: no masking) from ONE captured hipGraph.  The encoder is ~250 small kernels on 64
        tokens; at B = 1 their launch gaps dominate, so replaying a graph (static shapes, static buffers)
        is the MI355X-native way to run it until it gets fused kernels of its own.  The returned volumes
        are static buffers, overwritten by the next call."""
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("graph capture needs the GPU")
        xs = torch.zeros(batch, self.in_channel, 8, 8, device=dev)
        xt = torch.zeros_like(xs)
        state = {}

        def capture():
            with torch.no_grad():
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(2):  # warm-up: lazy library initialisation must not be captured
                        self.forward_2d3d(xs, xt, random_mask=False, mask_ratio=0.0)
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    out = self.forward_2d3d(xs, xt, random_mask=False, mask_ratio=0.0)
            state.update(graph=graph, out=out, epoch=packed_epoch(self))

        capture()

        @torch.no_grad()
        def run(layer4_src, layer4_tgt):
            # Parameters updated in place since the capture (optimizer.step()): refill the packed copies at their
            # captured addresses; parameters whose storage moved: capture again.
            if self._hip_2d3d_eligible(xs):
                _packed_aligner(self, dev)
                if packed_epoch(self) != state["epoch"]:
                    capture()
            xs.copy_(layer4_src)
            xt.copy_(layer4_tgt)
            state["graph"].replay()
            run.graph = state["graph"]
            return state["out"]

        run.graph = state["graph"]
        return run

    # ---- fused entry point (not in the reference: its call sites inline these three steps) ----
    def score_hypotheses(self, img_feat_src, img_feat_tgt, proposals, n_offset: int = 0, want_scores: bool = True):
        """forward_3d2d(tgt) + rotate_volume + forward_3d2d + score + running arg-max for every proposal in ONE launch
        (test_co3d.py:137-145, ``ops.verify_pair``).  Returns (scores (B,N) | None, packed best keys (B,))."""
        head = self.head_weights()
        if torch.is_grad_enabled() and any(t.requires_grad for t in (img_feat_src, img_feat_tgt) + tuple(head)):
            # training-shaped call: the one-launch step has no autograd edge; the differentiable pair of ops has
            # (forward_3d2d and the fused scorer both carry the HIP backward) -- nothing is detached silently
            feat_tgt = ops.forward_3d2d(img_feat_tgt, *head)
            return ops.score_hypotheses(img_feat_src, feat_tgt, proposals, *head, n_offset=n_offset, want_scores=True)
        return ops.verify_pair(img_feat_src, img_feat_tgt, proposals, *head, n_offset=n_offset, want_scores=want_scores)
