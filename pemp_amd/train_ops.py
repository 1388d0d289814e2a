"""Tensor-level wrappers over the training entry points of the C ABI (include/pemp_hip.h, "Training path").

Activations/gradients are NHWC fp32 views as in ``pemp_amd.ops``; 2-D ``[M, C]`` tensors are accepted
wherever the kernel only needs rows x channels.
"""
import ctypes as C

import torch

from . import _lib
from .ops import ConvDesc, CONV_STEM4, _p, _stream, _chk_dev, _ws, conv_out_size, _pool_out


def _rows(t, name):
    """-> (M, C, ld) of an NHWC view or a [M, C] matrix with unit channel stride."""
    if t.dtype != torch.float32 or t.stride(-1) != 1:
        raise ValueError(f"{name}: expected fp32 with unit channel stride")
    if t.dim() == 2:
        return t.shape[0], t.shape[1], (t.stride(0) if t.shape[0] > 1 else t.shape[1])
    if t.dim() == 4:
        from .ops import _nhwc
        n, h, w, c = t.shape
        return n * h * w, c, _nhwc(t, name)
    raise ValueError(f"{name}: expected 2-D or NHWC 4-D tensor")


def bn_stats(z, eps=1e-5, momentum=0.1, run_mean=None, run_var=None, ws_cache=None):
    """Batch mean and 1/sqrt(var+eps) per channel; updates running stats in place when given."""
    lib = _lib.load()
    _chk_dev(z, run_mean, run_var)
    m, c, ld = _rows(z, "z")
    mean = torch.empty(c, dtype=torch.float32, device=z.device)
    invstd = torch.empty(c, dtype=torch.float32, device=z.device)
    ws = _ws(lib.pemp_colsum_workspace_bytes(m, c), z.device, ws_cache, ("colsum", m, c))
    _lib.check(lib.pemp_bn_stats_f32(_p(z), ld, m, c, eps, momentum, _p(mean), _p(invstd), _p(run_mean), _p(run_var),
                                     _p(ws), ws.numel(), _stream()), "bn_stats")
    return mean, invstd


def _chk_part(part, what):
    if part.dtype != torch.float32 or not part.is_contiguous() or part.dim() != 3 or part.shape[1] != 2:
        raise ValueError(f"{what}: partials must be contiguous fp32 [row tiles, 2, C], got {tuple(part.shape)}")


def bn_stats_partials(part, m, eps=1e-5, momentum=0.1, run_mean=None, run_var=None):
    """bn_stats from the [row tiles, 2, C] partial sums a conv epilogue left (ops.conv2d_stats)."""
    lib = _lib.load()
    _chk_dev(part, run_mean, run_var)
    _chk_part(part, "bn_stats_partials")
    c = part.shape[2]
    mean = torch.empty(c, dtype=torch.float32, device=part.device)
    invstd = torch.empty(c, dtype=torch.float32, device=part.device)
    _lib.check(lib.pemp_bn_stats_partials_f32(_p(part), part.shape[0], m, c, eps, momentum, _p(mean), _p(invstd), _p(run_mean),
                                              _p(run_var), _stream()), "bn_stats_partials")
    return mean, invstd


def bn_fwd_partials(z, part, gamma, beta, out, eps=1e-5, momentum=0.1, run_mean=None, run_var=None, residual=None, relu=True,
                    mask=None):
    """bn_stats_partials + bn_apply in one call (pemp_bn_fwd_partials_f32): -> (out, mean, invstd)."""
    lib = _lib.load()
    _chk_dev(z, part, out, residual, mask, run_mean, run_var)
    _chk_part(part, "bn_fwd_partials")
    m, c, ldz = _rows(z, "z")
    _, _, ldy = _rows(out, "out")
    ldr = _rows(residual, "residual")[2] if residual is not None else 0
    if part.shape[2] != c:
        raise ValueError(f"bn_fwd_partials: partials have {part.shape[2]} channels, z has {c}")
    if mask is not None and (mask.dtype != torch.int32 or not mask.is_contiguous() or mask.numel() != m * (c // 32) or c % 32):
        raise ValueError(f"bn_fwd_partials: mask must be a contiguous int32 [{m}, {c}/32] tensor")
    mean = torch.empty(c, dtype=torch.float32, device=z.device)
    invstd = torch.empty(c, dtype=torch.float32, device=z.device)
    _lib.check(lib.pemp_bn_fwd_partials_f32(_p(z), ldz, _p(part), part.shape[0], m, c, eps, momentum, _p(gamma), _p(beta),
                                            _p(residual), ldr, _p(out), ldy, 1 if relu else 0, _p(mask), _p(mean), _p(invstd),
                                            _p(run_mean), _p(run_var), _stream()), "bn_fwd_partials")
    return out, mean, invstd


def bn_apply(z, mean, invstd, gamma, beta, out, residual=None, relu=True, mask=None):
    """``mask``: int32 [M, C/32] tensor that receives the sign bits of the result (bit c % 32 of mask[m, c // 32])."""
    lib = _lib.load()
    _chk_dev(z, out, residual, mask)
    m, c, ldz = _rows(z, "z")
    _, _, ldy = _rows(out, "out")
    ldr = _rows(residual, "residual")[2] if residual is not None else 0
    if mask is not None and (mask.dtype != torch.int32 or not mask.is_contiguous() or mask.numel() != m * (c // 32) or c % 32):
        raise ValueError(f"bn_apply: mask must be a contiguous int32 [{m}, {c}/32] tensor")
    _lib.check(lib.pemp_bn_apply_mask_f32(_p(z), ldz, _p(mean), _p(invstd), _p(gamma), _p(beta), _p(residual), ldr,
                                          _p(out), ldy, m, c, 1 if relu else 0, _p(mask), _stream()), "bn_apply")
    return out


def bn_apply_dropblock(z, mean, invstd, gamma, beta, out, dropblock):
    """BatchNorm apply (no residual, no ReLU) + the DropBlock2D behind it, one pass (pemp_bn_apply_dropblock_f32).
    ``dropblock`` = (mask fp32 [pixels], kept count int32 [1]) of ``dropblock_mask``; same arithmetic as bn_apply + pixel_scale."""
    lib = _lib.load()
    dmask, dcnt = dropblock
    _chk_dev(z, out, dmask, dcnt)
    m, c, ldz = _rows(z, "z")
    _, _, ldy = _rows(out, "out")
    if dmask.numel() != m or dmask.dtype != torch.float32 or not dmask.is_contiguous() or dcnt.dtype != torch.int32:
        raise ValueError("bn_apply_dropblock: mask must be a contiguous fp32 tensor with one entry per pixel, the count int32")
    _lib.check(lib.pemp_bn_apply_dropblock_f32(_p(z), ldz, _p(mean), _p(invstd), _p(gamma), _p(beta), _p(out), ldy, m, c,
                                               _p(dmask), _p(dcnt), _stream()), "bn_apply_dropblock")
    return out


def mask_supported(c):
    return c in (32, 64, 128, 256, 512, 1024)


def bn_bwd_partials(g, z, mean, invstd, gamma, part, dz, out=None):
    """Second half of the BatchNorm backward after ops.conv2d_bnbwd: -> (dgamma, dbeta); writes dz."""
    lib = _lib.load()
    _chk_dev(g, z, dz, part)
    m, c, ldg = _rows(g, "g")
    ldz = _rows(z, "z")[2]
    lddz = _rows(dz, "dz")[2]
    _chk_part(part, "bn_bwd_partials")
    if part.shape[2] != c:
        raise ValueError(f"bn_bwd_partials: partials have {part.shape[2]} channels, g has {c}")
    if out is None:
        dgamma = torch.empty(c, dtype=torch.float32, device=g.device)
        dbeta = torch.empty(c, dtype=torch.float32, device=g.device)
    else:
        dgamma, dbeta = out
    _lib.check(lib.pemp_bn_bwd_partials_f32(_p(g), ldg, _p(z), ldz, _p(mean), _p(invstd), _p(gamma), _p(part), part.shape[0],
                                            _p(dz), lddz, _p(dgamma), _p(dbeta), m, c, _stream()), "bn_bwd_partials")
    return dgamma, dbeta


def bn_bwd(dy, y, z, mean, invstd, gamma, dz, gout=None, relu=True, ws_cache=None, out=None, mask=None):
    """-> (dgamma, dbeta); writes dz (and gout = dy*(y>0), the gradient of the residual branch).
    ``out=(dgamma, dbeta)``: contiguous [C] tensors to write into (e.g. the flat-buffer gradient views).
    ``mask``: the sign bits of y from bn_apply(mask=...); y is then not read."""
    lib = _lib.load()
    _chk_dev(dy, y, z, dz, gout, mask)
    m, c, lddy = _rows(dy, "dy")
    ldy = _rows(y, "y")[2] if y is not None else 0
    ldz = _rows(z, "z")[2]
    lddz = _rows(dz, "dz")[2]
    ldg = _rows(gout, "gout")[2] if gout is not None else 0
    if out is not None:
        dgamma, dbeta = out
        if not (dgamma.is_contiguous() and dbeta.is_contiguous() and dgamma.numel() == c and dbeta.numel() == c):
            raise ValueError("bn_bwd: out tensors must be contiguous [C]")
    else:
        dgamma = torch.empty(c, dtype=torch.float32, device=dy.device)
        dbeta = torch.empty(c, dtype=torch.float32, device=dy.device)
    ws = _ws(lib.pemp_colsum_workspace_bytes(m, c), dy.device, ws_cache, ("colsum", m, c))
    if mask is not None and (mask.dtype != torch.int32 or not mask.is_contiguous() or mask.numel() != m * (c // 32) or c % 32):
        raise ValueError(f"bn_bwd: mask must be a contiguous int32 [{m}, {c}/32] tensor")
    _lib.check(lib.pemp_bn_bwd_mask_f32(_p(dy), lddy, _p(y), ldy, _p(mask if relu else None), _p(z), ldz, _p(mean), _p(invstd),
                                        _p(gamma), _p(dz), lddz, _p(gout), ldg, _p(dgamma), _p(dbeta), m, c, 1 if relu else 0,
                                        _p(ws), ws.numel(), _stream()), "bn_bwd")
    return dgamma, dbeta


def relu_bias_bwd(dy, y, g, add=None, relu=True, want_dbias=True, ws_cache=None, out=None):
    """g = (dy (+ add)) * (y > 0 if relu); returns dbias = column sums of g (or None); ``out``: contiguous [C]
    tensor to write dbias into (e.g. the bias gradient view of the flat buffer)."""
    lib = _lib.load()
    _chk_dev(dy, y, g, add)
    m, c, lddy = _rows(dy, "dy")
    ldy = _rows(y, "y")[2] if y is not None else 0
    lda = _rows(add, "add")[2] if add is not None else 0
    ldg = _rows(g, "g")[2]
    if out is not None and not (out.is_contiguous() and out.numel() == c):
        raise ValueError("relu_bias_bwd: out must be a contiguous [C] tensor")
    dbias = (out if out is not None else torch.empty(c, dtype=torch.float32, device=dy.device)) if want_dbias else None
    ws = _ws(lib.pemp_colsum_workspace_bytes(m, c), dy.device, ws_cache, ("colsum", m, c)) if want_dbias else None
    _lib.check(lib.pemp_relu_bias_bwd_f32(_p(dy), lddy, _p(y), ldy, _p(add), lda, _p(g), ldg, _p(dbias), m, c,
                                          1 if relu else 0, _p(ws), ws.numel() if ws is not None else 0, _stream()),
               "relu_bias_bwd")
    return dbias


from .ops import WGRAD_PICKS as _WGRAD_BLOCKS      # (layer geometry, input shape) -> (tile kind, block count) that measured fastest
WGRAD_BLOCK_CHOICES = (512, 768, 1024, 1536)


def conv_wgrad(x, g, p, dw, accumulate=False, ws_cache=None, variant=0, blocks=None):
    """dw (KRSC [Cout, Kpad_w]) (+)= wgrad of the conv described by ConvParams ``p`` (geometry only).
    For the stem ``dw`` has row length ceil(KH*KW*4 / 64) * 64.  ``variant`` = 1: the first-generation kernels
    (pointer-addressed; the library picks the buffer-addressed second generation where it applies, bit-identical).
    ``blocks``: how many blocks the pixel rows are split over (0: the library's 768; None: time WGRAD_BLOCK_CHOICES -- and,
    where both apply, the 128 x 128 and 64 x 64 tile kernels -- once per layer shape and keep the fastest; results of
    different splits differ by the rounding of the regrouped sum)."""
    lib = _lib.load()
    _chk_dev(x, g, dw)
    from .ops import _nhwc
    n, h, w, cin = x.shape
    ldx = _nhwc(x, "x")
    ho = conv_out_size(h, p.kh, p.stride, p.pad, p.dil)
    wo = conv_out_size(w, p.kw, p.stride, p.pad, p.dil)
    m, cout, ldg = _rows(g, "g")
    if m != n * ho * wo or cout != p.cout:
        raise ValueError(f"conv_wgrad: gradient has shape ({m},{cout}), expected ({n * ho * wo},{p.cout})")
    kpad = dw.shape[1]
    if dw.shape[0] != cout or not dw.is_contiguous():
        raise ValueError("conv_wgrad: dw must be contiguous [Cout, Kpad]")
    def launch(nb):          # nb: block count, or (tile kind 2 / 3, block count)
        kind, nb = nb if isinstance(nb, tuple) else (int(variant), nb)
        if variant:
            kind = int(variant)              # an explicit kernel generation wins over a remembered tile kind
        d = ConvDesc(n, h, w, cin, ldx, ho, wo, cout, ldg, p.kh, p.kw, p.stride, p.pad, p.dil, 0, kpad,
                     CONV_STEM4 if p.stem else 0, int(kind) | (int(nb) << 8))
        nbytes = lib.pemp_conv2d_wgrad_workspace_bytes(C.byref(d))
        ws = _ws(nbytes, x.device, ws_cache, ("wgrad", nbytes))
        _lib.check(lib.pemp_conv2d_wgrad_nhwc_f32(C.byref(d), _p(x), _p(g), _p(dw), 1 if accumulate else 0, _p(ws),
                                                  ws.numel(), _stream()), "conv_wgrad")

    if blocks is None:
        from . import ops
        # the pick depends on which kernel generation runs: the explicit ``variant`` and what decides the library's own choice
        # (geometry, strides) are part of the key -- a pick made for variant 1 must never be replayed for variant 0
        key = (cin, cout, p.kh, p.kw, p.stride, p.pad, p.dil, bool(p.stem), n, h, w, int(variant), ldx, ldg)
        blocks = _WGRAD_BLOCKS.get(key)
        if blocks is None:
            blocks = 0
            cands = list(WGRAD_BLOCK_CHOICES)
            if variant == 0 and not p.stem and cin % 128 == 0 and cout % 128 == 0:      # both tile sizes apply
                cands = [(k, nb) for k in (2, 3) for nb in WGRAD_BLOCK_CHOICES]
            if ops.PICK_HOOK is not None and not accumulate and not torch.cuda.is_current_stream_capturing():
                blocks = ops.PICK_HOOK("wgrad", list(cands), key)
                if blocks not in cands:
                    raise ValueError(f"PICK_HOOK returned {blocks!r}, not one of {cands}")
            elif ops.AUTOTUNE and not accumulate and m >= 4096 and not torch.cuda.is_current_stream_capturing():
                def timed(nb, reps=3):
                    launch(nb)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        launch(nb)
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1)
                ms = {nb: timed(nb) for nb in cands}
                for nb in cands:
                    ms[nb] = min(ms[nb], timed(nb))
                blocks = min(ms, key=ms.get)
            _WGRAD_BLOCKS[key] = blocks
            ops.save_picks()
    launch(blocks)
    return dw


def dgrad_mirror_table(layers, device):
    """``layers``: [(offset in floats, Cout, taps, Cin)] of the conv weights inside a flat parameter buffer -> (device int32
    table [L][6], total tiles) for ``dgrad_mirror``."""
    rows, first = [], 0
    for off, cout, taps, cin in layers:
        tci = (cin + 31) // 32
        rows.append([off, cout, taps, cin, first, tci])
        first += taps * ((cout + 31) // 32) * tci
    return torch.tensor(rows, dtype=torch.int32, device=device).contiguous(), first


def dgrad_mirror(params, mirror, table, total_tiles):
    """mirror[off : off + n] = the input-gradient KRSC weight ([Cin][taps flipped][Cout]) of every conv layer in ``table``,
    whose forward KRSC weight sits at params[off : off + n]: one launch per training step."""
    lib = _lib.load()
    _chk_dev(params, mirror, table)
    if params.numel() != mirror.numel() or not (params.is_contiguous() and mirror.is_contiguous()) or table.dtype != torch.int32:
        raise ValueError("dgrad_mirror: flat contiguous buffers of equal length and an int32 table required")
    _lib.check(lib.pemp_dgrad_mirror_f32(_p(params), _p(mirror), _p(table), table.shape[0], int(total_tiles), _stream()), "dgrad_mirror")
    return mirror


def dgrad_weight(w_krsc, kh, kw):
    """KRSC forward weight [Cout, KH*KW*Cin] -> the KRSC weight of the input-gradient conv
    [Cin, KH*KW*Cout] (taps flipped, channels transposed)."""
    cout = w_krsc.shape[0]
    cin = w_krsc.shape[1] // (kh * kw)
    w = w_krsc.view(cout, kh, kw, cin)
    return w.flip(1, 2).permute(3, 1, 2, 0).contiguous().view(cin, kh * kw * cout)


def maxpool_idx(x, k, s, p, ceil_mode=False):
    """nn.MaxPool2d forward that also records the winners -> (y, idx uint8 [n,ho,wo,c])."""
    lib = _lib.load()
    _chk_dev(x)
    if not x.is_contiguous():
        raise ValueError("maxpool_idx: contiguous NHWC tensor required")
    n, h, w, c = x.shape
    ho, wo = _pool_out(h, k, s, p, ceil_mode), _pool_out(w, k, s, p, ceil_mode)
    y = torch.empty((n, ho, wo, c), dtype=torch.float32, device=x.device)
    idx = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=x.device)
    _lib.check(lib.pemp_maxpool2d_idx_nhwc_f32(_p(x), _p(y), _p(idx), n, h, w, c, ho, wo, k, s, p, _stream()), "maxpool_idx")
    return y, idx


def maxpool_idx_bwd(idx, dy, in_hw, k, s, p):
    lib = _lib.load()
    _chk_dev(idx, dy)
    n, ho, wo, c = dy.shape
    h, w = in_hw
    if not (idx.is_contiguous() and dy.is_contiguous()) or idx.shape != dy.shape or idx.dtype != torch.uint8:
        raise ValueError("maxpool_idx_bwd: contiguous NHWC dy and matching uint8 idx required")
    dx = torch.empty((n, h, w, c), dtype=torch.float32, device=dy.device)
    _lib.check(lib.pemp_maxpool2d_idx_bwd_nhwc_f32(_p(idx), _p(dy), _p(dx), n, h, w, c, ho, wo, k, s, p, _stream()), "maxpool_idx_bwd")
    return dx


def maxpool_bwd(x, dy, k, s, p):
    lib = _lib.load()
    _chk_dev(x, dy)
    n, h, w, c = x.shape
    _, ho, wo, _ = dy.shape
    if not (x.is_contiguous() and dy.is_contiguous()):
        raise ValueError("maxpool_bwd: contiguous NHWC tensors required")
    dx = torch.empty_like(x)
    _lib.check(lib.pemp_maxpool2d_bwd_nhwc_f32(_p(x), _p(dy), _p(dx), n, h, w, c, ho, wo, k, s, p, _stream()), "maxpool_bwd")
    return dx


def scatter_strided(src, out_hw, s):
    lib = _lib.load()
    _chk_dev(src)
    n, hs, ws_, c = src.shape
    h, w = out_hw
    if not src.is_contiguous():
        raise ValueError("scatter_strided: contiguous NHWC source required")
    dst = torch.empty((n, h, w, c), dtype=torch.float32, device=src.device)
    _lib.check(lib.pemp_scatter_strided_nhwc_f32(_p(src), _p(dst), n, h, w, hs, ws_, c, s, _stream()), "scatter_strided")
    return dst


def gap_bwd_add(v, dst):
    """dst[n,i,:] += v[n,:] / HW."""
    lib = _lib.load()
    _chk_dev(v, dst)
    n, h, w, c = dst.shape
    _lib.check(lib.pemp_gap_bwd_add_nhwc_f32(_p(v.contiguous()), _p(dst), dst.stride(2), n, h * w, c, _stream()), "gap_bwd_add")
    return dst


class RandomStream:
    """(seed, offset) of the Philox stream the regulariser kernels draw from; every mask advances the offset,
    so successive layers and steps see different numbers and a re-seeded run repeats exactly."""

    def __init__(self, seed=0, device=None):
        self.seed, self.offset = int(seed) & (2 ** 64 - 1), 0
        # device-side step counter (added to the offset as step << 20 inside the kernels): lets a captured
        # hipGraph, whose kernel arguments are frozen, draw new numbers on every replay
        self.step = torch.zeros(1, dtype=torch.int64, device=device) if device is not None else None

    def next(self):
        self.offset += 1
        return self.seed, self.offset

    def begin_step(self):
        """Call once per training step (outside any graph capture)."""
        self.offset = 0
        if self.step is not None:
            self.step += 1


def dropblock_mask(n, h, w, drop_prob, block_size, rs, device, uniforms=None):
    """-> (mask fp32 [n,h,w] in {0,1}, kept_count int32 [1]) of one DropBlock2D call."""
    lib = _lib.load()
    mask = torch.empty((n, h, w), dtype=torch.float32, device=device)
    cnt = torch.empty(1, dtype=torch.int32, device=device)
    seed, off = rs.next()
    _lib.check(lib.pemp_dropblock_mask_f32(_p(mask), _p(cnt), _p(uniforms), n, h, w, float(drop_prob), int(block_size),
                                           seed, off, _p(rs.step), _stream()), "dropblock_mask")
    return mask, cnt


def pixel_scale(x, mask, cnt, out=None):
    """((x * mask[pixel]) * numel(mask)) / sum(mask): DropBlock2D forward and backward."""
    lib = _lib.load()
    _chk_dev(x, mask, cnt)
    m, c, ldx = _rows(x, "x")
    if mask.numel() != m:
        raise ValueError("pixel_scale: mask has a different pixel count")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device) if out is None else out
    _lib.check(lib.pemp_pixel_scale_f32(_p(x), ldx, _p(mask), _p(cnt), _p(out), _rows(out, "out")[2], m, c, _stream()),
               "pixel_scale")
    return out


def dropout2d_mask(n, c, p, rs, device, uniforms=None):
    lib = _lib.load()
    mask = torch.empty((n, c), dtype=torch.float32, device=device)
    seed, off = rs.next()
    _lib.check(lib.pemp_dropout2d_mask_f32(_p(mask), _p(uniforms), n, c, float(p), seed, off, _p(rs.step), _stream()),
               "dropout2d_mask")
    return mask


def channel_scale(x, mask, out=None):
    """x[n,h,w,c] * mask[n,c]: Dropout2d forward and backward."""
    lib = _lib.load()
    _chk_dev(x, mask)
    from .ops import _nhwc
    n, h, w, c = x.shape
    if tuple(mask.shape) != (n, c):
        raise ValueError("channel_scale: mask must be [N, C]")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device) if out is None else out
    _lib.check(lib.pemp_channel_scale_f32(_p(x), _nhwc(x, "x"), _p(mask), _p(out), _nhwc(out, "out"), n, h * w, c, _stream()),
               "channel_scale")
    return out


def cm_bias_bwd(colsum, feat, group, wext, dwext, dfeat_img, accumulate):
    """Backward of ``ops.cm_bias`` (training form, alpha = 1): writes dwext ([Cout,2] strided view of the weight
    gradient) and sets / adds to dfeat_img [N,2]."""
    lib = _lib.load()
    _chk_dev(colsum, feat, group, wext, dwext, dfeat_img)
    n, cout = colsum.shape
    if not colsum.is_contiguous() or wext.stride(1) != 1 or dwext.stride(1) != 1 or tuple(dfeat_img.shape) != (n, 2):
        raise ValueError("cm_bias_bwd: bad layouts")
    _lib.check(lib.pemp_cm_bias_bwd_f32(_p(colsum), _p(feat), _p(group), _p(wext), wext.stride(0), _p(dwext), dwext.stride(0),
                                        _p(dfeat_img), 1 if accumulate else 0, n, cout, _stream()), "cm_bias_bwd")


def cm_linear_bwd(dfeat_img, group, agg, lin_w, dlin_w, dlin_b):
    """Backward of ``ops.cm_linear``: writes dlin_w [2,2C], dlin_b [2]; returns dstat [N,2C]."""
    lib = _lib.load()
    _chk_dev(dfeat_img, group, agg, lin_w, dlin_w, dlin_b)
    n, (g, c2) = group.numel(), agg.shape
    if not (dlin_w.is_contiguous() and lin_w.is_contiguous() and agg.is_contiguous() and dfeat_img.is_contiguous()):
        raise ValueError("cm_linear_bwd: contiguous tensors required")
    dstat = torch.empty((n, c2), dtype=torch.float32, device=agg.device)
    _lib.check(lib.pemp_cm_linear_bwd_f32(_p(dfeat_img), _p(group), _p(agg), _p(lin_w), _p(dlin_w), _p(dlin_b), _p(dstat),
                                          n, g, c2, _stream()), "cm_linear_bwd")
    return dstat


def cm_bwd_add(x, mask, dstat, dx, argmax=None):
    """Backward of ``ops.cm_reduce``'s statistics: dx += mask * (dmean/HW + onehot(argmax) * dmax).
    x, dx: NHWC [N,h,w,C]; mask: the pooled mask cm_reduce returned [N,h,w]; dstat [N,2,C]; ``argmax`` int32 [N,C]
    from ``cm_reduce(want_argmax=True)`` skips the search for the maximal pixel."""
    lib = _lib.load()
    _chk_dev(x, mask, dstat, dx, argmax)
    from .ops import _nhwc
    n, h, w, c = x.shape
    if tuple(dx.shape) != (n, h, w, c) or tuple(dstat.shape) != (n, 2, c) or mask.numel() != n * h * w:
        raise ValueError("cm_bwd_add: shape mismatch")
    if argmax is not None:
        if argmax.dtype != torch.int32 or tuple(argmax.shape) != (n, c) or not argmax.is_contiguous():
            raise ValueError("cm_bwd_add: argmax must be contiguous int32 [N,C]")
        _lib.check(lib.pemp_cm_bwd_add_arg_f32(_p(mask.contiguous()), _p(dstat.contiguous()), _p(argmax), _p(dx),
                                               _nhwc(dx, "dx"), n, h * w, c, _stream()), "cm_bwd_add_arg")
        return dx
    _lib.check(lib.pemp_cm_bwd_add_f32(_p(x), _nhwc(x, "x"), _p(mask.contiguous()), _p(dstat.contiguous()), _p(dx),
                                       _nhwc(dx, "dx"), n, h * w, c, _stream()), "cm_bwd_add")
    return dx


def sgd_clip_step(params, grads, buf, max_norm, lr, momentum, weight_decay, first_step, grad_scale=1.0,
                  ws_cache=None, nesterov=False):
    """Flat-buffer clip_grad_norm_ + SGD step.  Returns the 1-element tensor holding ||grads||_2."""
    lib = _lib.load()
    _chk_dev(params, grads, buf)
    n = params.numel()
    if grads.numel() != n or buf.numel() != n or not (params.is_contiguous() and grads.is_contiguous() and buf.is_contiguous()):
        raise ValueError("sgd_clip_step: flat contiguous buffers of equal length required")
    norm = torch.empty(1, dtype=torch.float32, device=params.device)
    ws = _ws(lib.pemp_sgd_workspace_bytes(), params.device, ws_cache, ("sgd",))
    _lib.check(lib.pemp_sgd_clip_step_f32(_p(params), _p(grads), _p(buf), n, float(max_norm), float(lr), float(momentum),
                                          float(weight_decay), 1 if first_step else 0, float(grad_scale), 1 if nesterov else 0, _p(norm),
                                          _p(ws), ws.numel(), _stream()), "sgd_clip_step")
    return norm


def adam_clip_step(params, grads, exp_avg, exp_avg_sq, step, max_norm, lr, betas, eps, weight_decay, grad_scale=1.0, ws_cache=None):
    """Flat-buffer clip_grad_norm_ + torch.optim.Adam step (``step``: 1-based number of this update).  Returns the 1-element
    tensor holding ||grads||_2."""
    lib = _lib.load()
    _chk_dev(params, grads, exp_avg, exp_avg_sq)
    n = params.numel()
    if any(t.numel() != n or not t.is_contiguous() for t in (params, grads, exp_avg, exp_avg_sq)):
        raise ValueError("adam_clip_step: flat contiguous buffers of equal length required")
    norm = torch.empty(1, dtype=torch.float32, device=params.device)
    ws = _ws(lib.pemp_sgd_workspace_bytes(), params.device, ws_cache, ("sgd",))
    _lib.check(lib.pemp_adam_clip_step_f32(_p(params), _p(grads), _p(exp_avg), _p(exp_avg_sq), n, float(max_norm), float(lr),
                                           float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step),
                                           float(grad_scale), _p(norm), _p(ws), ws.numel(), _stream()), "adam_clip_step")
    return norm


def head_bwd_dlogits(sup_feat, qry_feat, sup_mask, ctr, fwd_ws, protos, dlogits, dfeat, B, S, p, dist_scalar,
                     ws_cache=None, map_full_res=False):
    """``head_bwd`` for an arbitrary gradient of the logits ``dlogits`` [B,2,Ho,Wo] (autograd's grad_output)."""
    lib = _lib.load()
    _chk_dev(sup_feat, qry_feat, sup_mask, ctr, fwd_ws, protos, dlogits, dfeat)
    from .ops import _nhwc
    ldf = _nhwc(sup_feat, "sup_feat")
    bs, h, w, c = sup_feat.shape
    H, W = sup_mask.shape[-2:]
    if dlogits.dtype != torch.float32 or not dlogits.is_contiguous() or dlogits.shape[:2] != (B, 2):
        raise ValueError("head_bwd_dlogits: dlogits must be contiguous fp32 [B,2,Ho,Wo]")
    ho, wo = dlogits.shape[-2:]
    ldd = _nhwc(dfeat, "dfeat")
    dctr = torch.empty((c, 2 * p), dtype=torch.float32, device=sup_feat.device) if p > 0 else None
    nbytes = lib.pemp_head_bwd_workspace_bytes(B, S, h * w, c, p)
    ws = _ws(nbytes, sup_feat.device, ws_cache, ("head_bwd", B, S, h, w, c, p))
    _lib.check(lib.pemp_head_bwd_dlogits_f32(_p(sup_feat), _p(qry_feat), ldf, _p(sup_mask), _p(ctr), _p(fwd_ws), _p(protos),
                                             _p(dlogits), _p(dfeat[:bs]), _p(dfeat[bs:]), ldd, _p(dctr), _p(ws), ws.numel(),
                                             B, S, h, w, H, W, ho, wo, c, p, 1 if map_full_res else 0, float(dist_scalar),
                                             _stream()), "head_bwd_dlogits")
    return dctr


def head_bwd(sup_feat, qry_feat, sup_mask, ctr, fwd_ws, protos, pred, target, stats, dfeat, B, S, p, dist_scalar,
             ws_cache=None, weight=None, map_full_res=False):
    """Gradient of the mean CE loss w.r.t. the features (written into ``dfeat`` [B*S + B, h, w, c], supports
    first) and w.r.t. ``ctr`` (returned, [c, 2p]; None for the plain-MAP head p == 0)."""
    lib = _lib.load()
    _chk_dev(sup_feat, qry_feat, sup_mask, ctr, fwd_ws, protos, pred, target, stats, dfeat)
    from .ops import _nhwc
    ldf = _nhwc(sup_feat, "sup_feat")
    bs, h, w, c = sup_feat.shape
    H, W = sup_mask.shape[-2:]
    ho, wo = target.shape[-2:]
    ldd = _nhwc(dfeat, "dfeat")
    dctr = torch.empty((c, 2 * p), dtype=torch.float32, device=sup_feat.device) if p > 0 else None
    nbytes = lib.pemp_head_bwd_workspace_bytes(B, S, h * w, c, p)
    ws = _ws(nbytes, sup_feat.device, ws_cache, ("head_bwd", B, S, h, w, c, p))
    _lib.check(lib.pemp_head_bwd_f32(_p(sup_feat), _p(qry_feat), ldf, _p(sup_mask), _p(ctr), _p(fwd_ws), _p(protos),
                                     _p(pred), _p(target), _p(weight), _p(stats), _p(dfeat[:bs]), _p(dfeat[bs:]), ldd, _p(dctr),
                                     _p(ws), ws.numel(), B, S, h, w, H, W, ho, wo, c, p, 1 if map_full_res else 0, float(dist_scalar),
                                     _stream()),
               "head_bwd")
    return dctr


# -- CANet head training (csrc/canet_bwd.hip) ---------------------------------------------------------------------------------
def canet_zterm_bwd(g, w_z, z, dw_z, dil, ws_cache=None):
    """Adjoint of ``ops.canet_zterm``: g NHWC [B,h,w,Cout] (the gradient at layer55's pre-activation), ``w_z`` / ``dw_z`` the z
    half of layer55's KRSC weight / weight gradient as [Cout,9,Cin] views of unit channel stride (column slices of the
    [Cout,9,Cin_total] matrix), z [B,Cin] -> (G [B,9,Cout] clipped tap sums of g, dz [B,Cin]); writes ``dw_z``."""
    lib = _lib.load()
    _chk_dev(g, w_z, z, dw_z)
    from .ops import _nhwc
    ldg = _nhwc(g, "g")
    b, h, w, cout = g.shape

    def rows(t, name):
        if t.dim() != 3 or t.dtype != torch.float32 or tuple(t.shape[:2]) != (cout, 9) or t.stride(2) != 1 or t.stride(0) != 9 * t.stride(1):
            raise ValueError(f"canet_zterm_bwd: {name} must be a fp32 [Cout,9,Cin] view with unit channel stride and dense rows")
        return t.stride(1)
    ldw = rows(w_z, "w_z")
    cin = w_z.shape[2]
    if rows(dw_z, "dw_z") != ldw or dw_z.shape[2] != cin:
        raise ValueError("canet_zterm_bwd: dw_z must be laid out as w_z")
    if tuple(z.shape) != (b, cin) or not z.is_contiguous() or z.dtype != torch.float32:
        raise ValueError(f"canet_zterm_bwd: z must be contiguous fp32 [{b},{cin}]")
    G = torch.empty((b, 9, cout), dtype=torch.float32, device=g.device)
    dz = torch.empty((b, cin), dtype=torch.float32, device=g.device)
    ws = _ws(lib.pemp_canet_zterm_bwd_workspace_bytes(b, h, w, cout), g.device, ws_cache, ("zterm_bwd", b, h, w, cout))
    _lib.check(lib.pemp_canet_zterm_bwd_f32(_p(g), ldg, _p(w_z), ldw, _p(z), _p(G), _p(dz), _p(dw_z), _p(ws), ws.numel(), b, h, w,
                                            cin, cout, int(dil), _stream()), "canet_zterm_bwd")
    return G, dz


def canet_support_vector_bwd(dz, sup_mask, S, df):
    """Adjoint of ``ops.canet_support_vector``: dz [B,C], sup_mask contiguous fp32 [B*S,2,H,W] -> writes df NHWC [B*S,h,w,C] (the
    support rows of the layer5-output gradient) = dz m / (S (sum m + 1e-5))."""
    lib = _lib.load()
    _chk_dev(dz, sup_mask, df)
    from .ops import _nhwc
    ldd = _nhwc(df, "df")
    n, h, w, c = df.shape
    if sup_mask.dim() != 4 or n % S or sup_mask.shape[0] != n or sup_mask.shape[1] != 2 or not sup_mask.is_contiguous() \
            or sup_mask.dtype != torch.float32:
        raise ValueError(f"canet_support_vector_bwd: sup_mask must be contiguous fp32 [B*S,2,H,W] for df {tuple(df.shape)}, S={S}")
    if tuple(dz.shape) != (n // S, c) or not dz.is_contiguous() or dz.dtype != torch.float32:
        raise ValueError("canet_support_vector_bwd: dz must be contiguous fp32 [B,C]")
    H, W = sup_mask.shape[-2:]
    _lib.check(lib.pemp_canet_support_vector_bwd_f32(_p(dz), _p(sup_mask), _p(df), ldd, n // S, S, h, w, H, W, c, _stream()),
               "canet_support_vector_bwd")
    return df


def canet_cls_bwd(dpred, x, weight, dx, dw, db, ws_cache=None):
    """Backward of a 1x1 conv to 2 classes: dpred contiguous [B,2,h,w], x NHWC [B,h,w,C], weight contiguous [2,C] -> writes dx
    NHWC [B,h,w,C], dw [2,C], db [2] (contiguous; e.g. the gradient views of the flat buffer)."""
    lib = _lib.load()
    _chk_dev(dpred, x, weight, dx, dw, db)
    from .ops import _nhwc
    ldx, lddx = _nhwc(x, "x"), _nhwc(dx, "dx")
    b, h, w, c = x.shape
    if tuple(dpred.shape) != (b, 2, h, w) or not dpred.is_contiguous() or dpred.dtype != torch.float32:
        raise ValueError(f"canet_cls_bwd: dpred must be contiguous fp32 [{b},2,{h},{w}]")
    if tuple(dx.shape) != tuple(x.shape):
        raise ValueError("canet_cls_bwd: dx must have x's shape")
    for t, n in ((weight, 2 * c), (dw, 2 * c), (db, 2)):
        if t.numel() != n or not t.is_contiguous() or t.dtype != torch.float32:
            raise ValueError("canet_cls_bwd: weight / dw must be contiguous fp32 [2,C], db contiguous fp32 [2]")
    ws = _ws(lib.pemp_canet_cls_bwd_workspace_bytes(b * h * w, c), x.device, ws_cache, ("cls_bwd", b * h * w, c))
    _lib.check(lib.pemp_canet_cls_bwd_f32(_p(dpred), _p(x), ldx, _p(weight), _p(dx), lddx, _p(dw), _p(db), _p(ws), ws.numel(),
                                          b, h * w, c, _stream()), "canet_cls_bwd")
    return dx


def upsample_ce_bwd(pred=None, target=None, stats=None, weight=None, dlogits=None, out=None, low_hw=None):
    """The first stage of ``head_bwd`` on its own -> dpred [B,2,h,w]: the adjoint of the bilinear (align_corners) upsample of
    ``pred`` [B,2,h,w] to the target's size, applied to the mean-CE gradient from (pred, target int64 [B,Ho,Wo], stats of
    ``ops.eval_tail``, optional ``weight`` map) or to a given ``dlogits`` [B,2,Ho,Wo] (then ``low_hw`` = (h, w))."""
    lib = _lib.load()
    _chk_dev(pred, target, stats, weight, dlogits, out)
    if dlogits is not None:
        if dlogits.dim() != 4 or dlogits.shape[1] != 2 or not dlogits.is_contiguous() or dlogits.dtype != torch.float32 or low_hw is None:
            raise ValueError("upsample_ce_bwd: dlogits must be contiguous fp32 [B,2,Ho,Wo] and comes with low_hw")
        b, (ho, wo), (h, w), dev = dlogits.shape[0], dlogits.shape[-2:], low_hw, dlogits.device
        pred = target = stats = weight = None
    else:
        if pred is None or target is None or stats is None:
            raise ValueError("upsample_ce_bwd: (pred, target, stats) or dlogits is needed")
        if pred.dim() != 4 or pred.shape[1] != 2 or not pred.is_contiguous() or pred.dtype != torch.float32:
            raise ValueError("upsample_ce_bwd: pred must be contiguous fp32 [B,2,h,w]")
        b, _, h, w = pred.shape
        if target.dtype != torch.int64 or not target.is_contiguous() or target.dim() != 3 or target.shape[0] != b:
            raise ValueError("upsample_ce_bwd: target must be contiguous int64 [B,Ho,Wo]")
        ho, wo = target.shape[-2:]
        if stats.dtype != torch.float64 or tuple(stats.shape) != (b, 8) or not stats.is_contiguous():
            raise ValueError("upsample_ce_bwd: stats must be the contiguous float64 [B,8] of eval_tail")
        if weight is not None and (weight.dtype != torch.float32 or not weight.is_contiguous() or tuple(weight.shape) != (b, ho, wo)):
            raise ValueError("upsample_ce_bwd: weight must be contiguous fp32 [B,Ho,Wo]")
        dev = pred.device
    if out is None:
        out = torch.empty((b, 2, int(h), int(w)), dtype=torch.float32, device=dev)
    if tuple(out.shape) != (b, 2, int(h), int(w)) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("upsample_ce_bwd: out must be contiguous fp32 [B,2,h,w]")
    _lib.check(lib.pemp_upsample_ce_bwd_f32(_p(pred), _p(target), _p(weight), _p(stats), _p(dlogits), _p(out), b, int(h), int(w),
                                            int(ho), int(wo), _stream()), "upsample_ce_bwd")
    return out


# -- PFENet head training (csrc/pfenet_bwd.hip) -------------------------------------------------------------------------------
def weighted_gap_bwd(dvec, mask, S, df):
    """Adjoint of ``ops.weighted_gap``: dvec contiguous [B,C], mask contiguous fp32 [B*S,h,w] -> writes df NHWC [B*S,h,w,C] (the
    support rows of the down_supp-output gradient) = dvec m / (sum m + 5e-4) / S."""
    lib = _lib.load()
    _chk_dev(dvec, mask, df)
    from .ops import _nhwc
    ldd = _nhwc(df, "df")
    n, h, w, c = df.shape
    if n % S or tuple(mask.shape) != (n, h, w) or not mask.is_contiguous() or mask.dtype != torch.float32:
        raise ValueError(f"weighted_gap_bwd: mask must be contiguous fp32 [B*S,h,w] for df {tuple(df.shape)}, S={S}")
    if tuple(dvec.shape) != (n // S, c) or not dvec.is_contiguous() or dvec.dtype != torch.float32:
        raise ValueError("weighted_gap_bwd: dvec must be contiguous fp32 [B,C]")
    _lib.check(lib.pemp_weighted_gap_bwd_f32(_p(dvec), _p(mask), _p(df), ldd, n // S, S, h, w, c, _stream()), "weighted_gap_bwd")
    return df


def _bin_tables(gs, name, n, c):
    """ctypes tables (pointers, pixel strides, heights, widths) of NHWC views gs[k] [n,h_k,w_k,c]."""
    from .ops import _nhwc
    nb = len(gs)
    if not 1 <= nb <= 4:
        raise ValueError(f"{name}: 1 to 4 bins per call, got {nb}")
    ld = []
    for g in gs:
        ld.append(_nhwc(g, "g"))
        if g.shape[0] != n or g.shape[3] != c:
            raise ValueError(f"{name}: every g must be [{n},h,w,{c}], got {tuple(g.shape)}")
    ints = C.c_int * nb
    return nb, (C.c_void_p * nb)(*[g.data_ptr() for g in gs]), ints(*ld), ints(*[g.shape[1] for g in gs]), ints(*[g.shape[2] for g in gs])


def adaptive_avgpool_bwd_multi(gs, dx):
    """Sum of the adjoints of ``ops.adaptive_avgpool(x, bin_k)`` for up to four bins: gs[k] NHWC [N,bin_k,bin_k',C] -> writes dx NHWC
    [N,H,W,C] (a channel slice of a wider buffer is fine); dx is written once, not accumulated."""
    lib = _lib.load()
    _chk_dev(dx, *gs)
    from .ops import _nhwc
    lddx = _nhwc(dx, "dx")
    n, h, w, c = dx.shape
    nb, ptrs, ld, bh, bw = _bin_tables(gs, "adaptive_avgpool_bwd_multi", n, c)
    _lib.check(lib.pemp_adaptive_avgpool_bwd_multi_nhwc_f32(nb, ptrs, ld, bh, bw, _p(dx), lddx, n, h, w, c, _stream()),
               "adaptive_avgpool_bwd_multi")
    return dx


def resize_bilinear_ac_bwd(dy, size=None, add=None, out=None):
    """Adjoint of ``ops.resize_bilinear_ac``: dy [N,ho,wo,C] (the gradient at the resized map) -> dx [N,hi,wi,C] = add + A^T dy, with
    ``size`` = (hi, wi) or taken from ``out``.  Views with any (image, pixel, channel) strides, as the forward takes; ``add`` may be
    ``out`` itself.  ``out`` None: a new contiguous NHWC tensor."""
    lib = _lib.load()
    _chk_dev(dy, add, out)
    from .ops import _strides4
    n, ho, wo, c = dy.shape
    if out is None:
        hi, wi = (size, size) if isinstance(size, int) else size
        out = torch.empty((n, hi, wi, c), dtype=torch.float32, device=dy.device)
    hi, wi = out.shape[1:3]
    if tuple(out.shape) != (n, hi, wi, c) or (size is not None and (hi, wi) != ((size, size) if isinstance(size, int) else tuple(size))):
        raise ValueError(f"resize_bilinear_ac_bwd: out {tuple(out.shape)} does not fit dy {tuple(dy.shape)} and size {size}")
    if add is not None and tuple(add.shape) != tuple(out.shape):
        raise ValueError("resize_bilinear_ac_bwd: add must have out's shape")
    yn, yp, yc = _strides4(dy, "dy")
    xn, xp, xc = _strides4(out, "out")
    an, ap, ac = _strides4(add, "add") if add is not None else (0, 0, 0)
    _lib.check(lib.pemp_resize_bilinear_ac_bwd_nhwc_f32(_p(dy), yn, yp, yc, _p(add), an, ap, ac, _p(out), xn, xp, xc, n, c, hi, wi, ho,
                                                        wo, _stream()), "resize_bilinear_ac_bwd")
    return out


def pfenet_merge_support_bwd(gs, w_s, svec, dw_s, ws_cache=None):
    """The support half of PFENet's ``init_merge`` convs, all bins at once: gs[k] NHWC [B,bin_k,bin_k,Cout] (the gradient at conv
    k's pre-activation), w_s[k] / dw_s[k] the support columns of conv k's weight / weight gradient as [Cout,Cin] views of unit
    column stride and one common row stride, svec contiguous [B,Cin] -> dsvec [B,Cin]; writes every dw_s[k]."""
    lib = _lib.load()
    _chk_dev(svec, *gs, *w_s, *dw_s)
    b, cin = svec.shape
    if not svec.is_contiguous() or svec.dtype != torch.float32:
        raise ValueError("pfenet_merge_support_bwd: svec must be contiguous fp32 [B,Cin]")
    cout = gs[0].shape[3]
    nb, ptrs, ld, bh, bw = _bin_tables(gs, "pfenet_merge_support_bwd", b, cout)
    if len(w_s) != nb or len(dw_s) != nb:
        raise ValueError("pfenet_merge_support_bwd: one weight and one weight gradient per bin")
    ldw = w_s[0].stride(0)
    for t in (*w_s, *dw_s):
        if t.dim() != 2 or t.dtype != torch.float32 or tuple(t.shape) != (cout, cin) or t.stride(1) != 1 or t.stride(0) != ldw:
            raise ValueError(f"pfenet_merge_support_bwd: weights must be fp32 [{cout},{cin}] views with unit column stride and one "
                             "row stride")
    arr = C.c_void_p * nb
    dsvec = torch.empty((b, cin), dtype=torch.float32, device=svec.device)
    ws = _ws(lib.pemp_pfenet_merge_support_bwd_workspace_bytes(nb, b, cout), svec.device, ws_cache, ("merge_s_bwd", nb, b, cout))
    _lib.check(lib.pemp_pfenet_merge_support_bwd_f32(nb, ptrs, ld, bh, bw, arr(*[t.data_ptr() for t in w_s]),
                                                     arr(*[t.data_ptr() for t in dw_s]), ldw, _p(svec), _p(dsvec), _p(ws), ws.numel(),
                                                     b, cin, cout, _stream()), "pfenet_merge_support_bwd")
    return dsvec


# -- RPMMs head training (csrc/rpmms_bwd.hip) ---------------------------------------------------------------------------------
def _rpmms_operands(who, base, bias, taps, mult, mu=None):
    from .ops import RPMMS_COLS, _nhwc
    ldb = _nhwc(base, "base")
    b, h, w, c = base.shape
    for t, shape, name in ((bias, (c,), "bias"), (taps, (b, RPMMS_COLS, 9, c), "taps"), (mult, (b, RPMMS_COLS, c), "mult"),
                           (mu, (b, 2, RPMMS_COLS, c), "mu")):
        if t is not None and (tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != torch.float32):
            raise ValueError(f"{who}: {name} must be contiguous fp32 {list(shape)}, got {tuple(t.shape)}")
    return ldb, b, h, w, c


def rpmms_proto_sum_train(wz, mu, base, bias, mult, out, dil=2, taps=None):
    """``ops.rpmms_proto_sum`` in train() mode (rpmms.py:237-244 with layer55's Dropout2d drawn once per prototype): ``mult``
    contiguous fp32 [B,10,256], column i's multiplier (0 or 1 / (1 - p)) on its ReLU output before the sum over the mixture's
    columns; the other operands as there.  With every multiplier 1.0 the result is ``ops.rpmms_proto_sum``'s, bit for bit.
    -> (out, taps): ``taps`` [B,10,9,256] is an operand of the backward."""
    from .ops import RPMMS_COLS, _rpmms_groups_out
    lib = _lib.load()
    _chk_dev(wz, mu, base, bias, mult, out, taps)
    b, h, w, c = base.shape
    if taps is None:
        taps = torch.empty((b, RPMMS_COLS, 9, c), dtype=torch.float32, device=base.device)
    ldb = _rpmms_operands("rpmms_proto_sum_train", base, bias, taps, mult, mu)[0]
    if tuple(wz.shape) != (9, c, c) or not wz.is_contiguous() or wz.dtype != torch.float32:
        raise ValueError(f"rpmms_proto_sum_train: wz must be contiguous fp32 [9,{c},{c}]")
    ldo, gstride = _rpmms_groups_out("rpmms_proto_sum_train", out, b, h, w, c, c)
    _lib.check(lib.pemp_rpmms_proto_sum_train_f32(_p(wz), _p(mu), _p(base), ldb, _p(bias), _p(mult), _p(taps), _p(out), ldo, gstride,
                                                  b, h, w, c, int(dil), _stream()), "rpmms_proto_sum_train")
    return out, taps


def rpmms_proto_bwd_work_floats(B, h, w, C=256):
    """Size of ``rpmms_proto_sum_bwd``'s workspace (include/pemp_hip.h: B x 10 columns x G pixel blocks x 9 taps x C partial
    sums, G = min(16, ceil(h w / 4)))."""
    from .ops import RPMMS_COLS
    return B * RPMMS_COLS * min(16, -(-(h * w) // 4)) * 9 * C


def rpmms_proto_sum_bwd(dout, base, bias, taps, mult, dil=2, mu=None, dw_z=None, dbias=None, dbase=None, work=None, ws_cache=None):
    """Adjoint of ``rpmms_proto_sum_train``: dout fp32 [3,B,h,w,ld >= 256] (the gradients at the three mixture outputs), base, bias,
    taps, mult as in the forward -> (dbase NHWC [B,h,w,256], G [B,10,9,256]: per column and tap the sum of the column's gated
    gradient over the pixels whose tap source lies inside the image).  With ``mu`` [B,2,10,256] and ``dw_z``, the prototype half
    of layer55's KRSC weight gradient as a [Cout,9,Cin] view of unit channel stride (a column slice of [Cout,9,Cin_total]), dW_z
    = sum_b sum_i G[b,i] (x) mu[b,0,i] is written there; ``dbias`` [256] takes the sum of dbase over images and pixels.  ``work``: a
    fp32 buffer of ``rpmms_proto_bwd_work_floats`` elements (default: taken from ``ws_cache`` or allocated)."""
    from .ops import RPMMS_COLS, _nhwc, _rpmms_groups_out
    lib = _lib.load()
    _chk_dev(dout, base, bias, taps, mult, mu, dw_z, dbias, dbase, work)
    ldb, b, h, w, c = _rpmms_operands("rpmms_proto_sum_bwd", base, bias, taps, mult, mu)
    ldd, gstride = _rpmms_groups_out("rpmms_proto_sum_bwd", dout, b, h, w, c, c)
    if dbase is None:
        dbase = torch.empty((b, h, w, c), dtype=torch.float32, device=base.device)
    if tuple(dbase.shape) != (b, h, w, c):
        raise ValueError(f"rpmms_proto_sum_bwd: dbase {tuple(dbase.shape)} != {(b, h, w, c)}")
    lddb = _nhwc(dbase, "dbase")
    ldw = 0
    if dw_z is not None:
        if mu is None:
            raise ValueError("rpmms_proto_sum_bwd: dw_z needs mu")
        if dw_z.dim() != 3 or dw_z.dtype != torch.float32 or tuple(dw_z.shape) != (c, 9, c) or dw_z.stride(2) != 1 \
                or dw_z.stride(0) != 9 * dw_z.stride(1):
            raise ValueError("rpmms_proto_sum_bwd: dw_z must be a fp32 [256,9,256] view with unit channel stride and dense rows")
        ldw = dw_z.stride(1)
    if dbias is not None and (tuple(dbias.shape) != (c,) or not dbias.is_contiguous() or dbias.dtype != torch.float32):
        raise ValueError(f"rpmms_proto_sum_bwd: dbias must be contiguous fp32 [{c}]")
    need = rpmms_proto_bwd_work_floats(b, h, w, c)
    if work is None:
        work = _ws(4 * need, base.device, ws_cache, ("rpmms_proto_bwd", b, h, w)).view(torch.float32)
    if work.numel() < need or not work.is_contiguous() or work.dtype != torch.float32:
        raise ValueError(f"rpmms_proto_sum_bwd: work must be a contiguous fp32 buffer of at least {need} elements")
    G = torch.empty((b, RPMMS_COLS, 9, c), dtype=torch.float32, device=base.device)
    _lib.check(lib.pemp_rpmms_proto_sum_bwd_f32(_p(dout), ldd, gstride, _p(base), ldb, _p(bias), _p(taps), _p(mult), _p(mu), _p(dbase),
                                                lddb, _p(G), _p(dw_z), ldw, _p(dbias), _p(work), work.numel(), b, h, w, c, int(dil),
                                                _stream()), "rpmms_proto_sum_bwd")
    return dbase, G


def rpmms_history_bwd(dh, prob, dpred):
    """Adjoint of the two-class softmax that turns a pass's logits into the next pass's history (rpmms.py:250-251,285): dh NHWC
    [B,h,w,2] (a channel slice is fine: the gradient at the two history channels), prob contiguous fp32 [B,2,h,w] (the softmax
    that was fed forward) -> dpred [B,2,h,w] += prob_k (dh_k - sum_j prob_j dh_j), in place."""
    from .ops import _nhwc
    lib = _lib.load()
    _chk_dev(dh, prob, dpred)
    ldh = _nhwc(dh, "dh")
    b, h, w, c = dh.shape
    for t, name in ((prob, "prob"), (dpred, "dpred")):
        if tuple(t.shape) != (b, 2, h, w) or not t.is_contiguous() or t.dtype != torch.float32:
            raise ValueError(f"rpmms_history_bwd: {name} must be contiguous fp32 [{b},2,{h},{w}], got {tuple(t.shape)}")
    if c != 2:
        raise ValueError("rpmms_history_bwd: dh must hold the two history channels")
    _lib.check(lib.pemp_rpmms_history_bwd_f32(_p(dh), ldh, _p(prob), _p(dpred), b, h * w, _stream()), "rpmms_history_bwd")
    return dpred
