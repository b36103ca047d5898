"""Plain references, the clip_embed bound, reference mutants and case lists of everything that decides which pixel or CLIP feature lands
in which operand row: csrc/rowops.hip im2col / clip_embed / hd_gather / clip_tokens / llava_pack, csrc/rowops_qwen.hip qwen_patch_gather,
and the host plans behind them (csrc/engine.hip plan_hd_sample / plan_llava_sample, csrc/qwen.hip qwen_vision_plan), for
tests/test_vision_reference.py (CPU) and tests/test_gpu_vision.py (MI355X).  Built like helpers/plan_ref.py and helpers/rowops_ref.py.

The references restate none of the kernels' index arithmetic: the HD transform is the reference model's reshape / permute
(modeling_phi3_v.py:305-362), unpad and newline are slices and concatenations (modeling_llava_next.py pack_image_features / unpad_image),
im2col is torch's unfold of the conv2d the patch embedding is, the window plan sorts merge units by (window row, window column, y, x).
They are checked against the real programs through the fixtures tests/golden/make_vision_goldens.py records (source maps of index-valued
features), and against synth's restatements.

Copies.  im2col, hd_gather, clip_tokens, llava_pack and qwen_patch_gather move values and round them once to the operand type
([hi | lo]: hi = RNE(v), lo = RNE(v - hi), plan_ref._encode): no other arithmetic, so they are compared BIT FOR BIT.
clip_embed.  v = src + pos one rounding (u32 |v|), then the LayerNorm of rowops_ref's 4-wide row kernel: the row sum and the sum of
squares by lane_sum(64 lanes, float4 chunks summed first) in the kernel's order, mean and variance one rounding each, + eps one, rsqrtf
propagated through its graph + RSQRT_ULP ulp, (a * rstd) * w two roundings, + b one.  The error of v is carried through every step.  Worst
case, every rounding at its maximum and one sign: no margin factor.
"""
import hashlib
import types

import numpy as np
import torch

from .gemm_ref import TDT, U32  # noqa: F401
from .plan_ref import _encode
from .rowops_ref import RSQRT_ULP, _rsqrt, f32, lane_sum, ratio  # noqa: F401

F32, F64 = torch.float32, torch.float64
LR_BACKBONE_PHI3V, LR_BACKBONE_LLAVA_NEXT = 0, 1

MUTANTS = {
    "hd_gather": ("di_dj_swapped", "sub_separator_at_column_0", "global_separator_one_row_early", "crop_index_hc_for_wc", "cls_not_skipped",
                  "global_crop_from_crop0_plus_1"),
    "llava_pack": ("newline_before_row", "r0_used_for_columns", "crop_index_gh_for_gw", "base_crop_from_crop0_plus_1", "y_x_in_crop_swapped"),
    "im2col": ("ky_kx_swapped", "channel_minor_k", "crop_src_ignored", "pad_not_zero", "lo_of_unrounded_hi"),
    "clip_embed": ("position_t_minus_1", "cls_position_on_every_row", "crop_stride_T", "unbiased_variance"),
    "clip_tokens": ("cls_kept",),
    "qwen_patch_gather": ("identity_order", "pad_not_zero", "bf16_read_as_fp16"),
    "qwen_window_plan": ("no_empty_extra_window", "column_major_windows", "hw_without_merge_offset", "slot2row_in_window_order", "items_chunk_64"),
    "llava_plan": ("floor_not_round7", "tie_broken_by_first", "aspect_test_ge"),
}
DTS = ("bf16", "f16")


def digest(rows):
    """The fixture's digest of an integer list: sha256 of its little-endian int32 bytes, 16 hex digits."""
    return hashlib.sha256(np.asarray(rows, "<i4").tobytes()).hexdigest()[:16]


# ---------------------------------------------------------------------------------------------------------------------------------------
# host plans
# ---------------------------------------------------------------------------------------------------------------------------------------
LLAVA_PINPOINT_GRIDS = ((1, 2), (2, 1), (2, 2), (3, 1), (1, 3))     # llava-v1.6 image_grid_pinpoints in crops (h, w)


def pinpoints(crop):
    return [(a * crop, b * crop) for a, b in LLAVA_PINPOINT_GRIDS]


def pinpoints_reordered(crop):
    """The same resolutions with 2 x 2 in front: a tall or wide image then ties 2 x 2 with 2 x 1 / 1 x 2 on the effective resolution, and
    only the waste picks the smaller grid (in the checkpoint's own order the first of such a tie is also the least wasteful)."""
    return [(a * crop, b * crop) for a, b in ((2, 2), (1, 2), (2, 1), (3, 1), (1, 3))]


REORDERED_SIZES = lambda c: [(2 * c + 7, c - 5), (c - 5, 2 * c + 7), (3 * c // 2, c // 2), (c // 2, 3 * c // 2), (c, c), (2 * c, 2 * c - 1)]
# sizes at which int(x) and int(round(x, 7)) part: the product that should be a whole number of rows or columns comes out one ulp short
ROUND7_SIZES = {336: [(55, 176), (88, 55), (176, 110), (47, 1128)], 56: [(47, 188), (188, 47), (49, 588)], 28: [(49, 294), (196, 147)]}
# aspect_test_ge cannot be caught: w / h == cw / ch holds for integers below 2^12 only when w ch == h cw exactly, and then either branch finds
# the whole extent (h (cw / w) is within two ulp of ch, which round(x, 7) restores) and pads by 0.  The CPU file checks exactly that.
# no_empty_extra_window cannot be caught either: an empty window holds no row and yields no work item (qwen_window_plan_ref).
EQUIVALENT_MUTANTS = {"llava_plan": ("aspect_test_ge",), "qwen_window_plan": ("no_empty_extra_window",)}


def llava_select(h, w, pins, mutant=None):
    """transformers select_best_resolution: the largest effective resolution, then the least waste, the first on a full tie."""
    best, key = None, None
    for ph, pw in pins:
        s = min(pw / w, ph / h)
        eff = min(int(w * s) * int(h * s), w * h)
        k = (eff, 0) if mutant == "tie_broken_by_first" else (eff, -(ph * pw - eff))
        if key is None or k > key:
            best, key = (ph, pw), k
    return best


def llava_plan_ref(h, w, pins, crop, g, mutant=None):
    """(gh, gw, r0, r1, c0, c1, crops, rows) of one image: the anyres grid, the rows and columns of the (gh g) x (gw g) feature map that
    survive unpad_image -- new extent int(round(x, 7)) -- and the counts: 1 + gh gw crops, g g + rows (cols + 1) image rows."""
    bh, bw = llava_select(h, w, pins, mutant)
    gh, gw = bh // crop, bw // crop
    ch, cw = gh * g, gw * g
    cut = (lambda x: int(x)) if mutant == "floor_not_round7" else (lambda x: int(round(x, 7)))
    r0, r1, c0, c1 = 0, ch, 0, cw
    wide = (w / h >= cw / ch) if mutant == "aspect_test_ge" else (w / h > cw / ch)
    if wide:
        pad = (ch - cut(h * (cw / w))) // 2
        r0, r1 = pad, ch - pad
    else:
        pad = (cw - cut(w * (ch / h))) // 2
        c0, c1 = pad, cw - pad
    return gh, gw, r0, r1, c0, c1, 1 + gh * gw, g * g + (r1 - r0) * (c1 - c0 + 1)


def hd_plan_ref(h, w, crop, g):
    """(hc, wc, crops, rows) of one Phi-3-V image whose padded size is (h, w): rows counted off the shapes of hd_feature_transform."""
    hc, wc, g2 = h // crop, w // crop, g // 2
    return hc, wc, hc * wc + 1, (hc * g2) * (wc * g2 + 1) + 1 + g2 * (g2 + 1)


def llava_sizes(crop):
    """(h, w) list of the LLaVA fixtures and kernel cases at crop size `crop`: square, portrait, landscape, both unpad branches, pad = 0,
    the extreme strips, tiny images, and the two sizes on each side of every switch of select_best_resolution met while sweeping w at
    fixed h and h at fixed w (first occurrence of each ordered pair of resolutions per sweep direction)."""
    c, pins = crop, pinpoints(crop)
    out = [(c, c), (2 * c, 2 * c), (3 * c, 2 * c), (2 * c, 3 * c), (c, 2 * c), (2 * c, c), (3 * c, c), (c, 3 * c),      # pad = 0 on the exact grids
           (c + c // 3, 2 * c + c // 2), (2 * c + c // 2, c + c // 3), (c // 2 + 1, 2 * c - 3), (2 * c - 3, c // 2 + 1),
           (5 * c // 4, 5 * c // 4 - 1), (5 * c // 4 - 1, 5 * c // 4), (1, 2000), (2000, 1), (3, 1), (1, 3), (5, 1), (10, 1), (1, 1), (7, 9)]
    out += ROUND7_SIZES.get(crop, [])
    seen = set()
    for fixed in (c // 2, c, 3 * c // 2 + 1, 2 * c + 5):
        for swap in (False, True):
            prev = None
            for v in range(1, 5 * c):
                hw = (v, fixed) if swap else (fixed, v)
                cur = llava_select(*hw, pins)
                if prev is not None and cur != prev and (swap, prev, cur) not in seen:
                    seen.add((swap, prev, cur))
                    out += [((v - 1, fixed) if swap else (fixed, v - 1)), hw]
                prev = cur
    uniq = []
    for s in out:
        if s not in uniq:
            uniq.append(s)
    return uniq


def llava_sweep():
    hs = list(range(1, 40)) + list(range(40, 2100, 13))
    ws = list(range(1, 40)) + list(range(40, 2100, 11))
    return [(h, w) for h in hs for w in ws]


HD_GRIDS = ((1, 1), (1, 2), (2, 1), (2, 3), (3, 1), (4, 4))
HD_BATCH = ((2, 3), (3, 1))


def qwen_window_plan_ref(grids, merge, ws, mutant=None):
    """The vision plan of lr_forward_qwen for grids [(gh, gw)] in patches: merge units sorted by (window row, window column, y, x), every
    unit followed by its merge x merge patches in the processor's order [lh, lw, m, m].  Returns a namespace of int arrays: src [N] (the
    processor row of every row in window order), hw [N, 2], slot2row [N / unit], items_win / items_full [*, 4] = (first row, length,
    128-query tile, 0), imgs [n, 4] = (lh, lw, advance, first unit), counts (N, nwin, nfull, max_seg), and cu: the cumulative row count
    behind every window that holds rows (transformers' cu_window_seqlens: the padded window grid has a whole extra window row / column when
    the grid divides evenly, and unique_consecutive drops what stays empty -- so a plan without the extra windows differs in nothing)."""
    unit = merge * merge
    src, hw, items_win, items_full, imgs, cu_raw = [], [], [], [], [], [0]
    slot2row = {}
    mbase, max_seg = 0, 0
    chunk = 64 if mutant == "items_chunk_64" else 128
    for gh, gw in grids:
        lh, lw = gh // merge, gw // merge
        imgs.append((lh, lw, max(gh, gw) // merge, mbase))
        units = [(y, x) for y in range(lh) for x in range(lw)]
        if mutant == "column_major_windows":
            units.sort(key=lambda p: (p[1] // ws, p[0] // ws, p[0], p[1]))
        else:
            units.sort(key=lambda p: (p[0] // ws, p[1] // ws, p[0], p[1]))
        row_img = len(src)
        for i, (y, x) in enumerate(units):
            u = mbase + y * lw + x
            if mutant == "slot2row_in_window_order":
                slot2row[mbase + i] = u
            else:
                slot2row[u] = len(src) // unit
            for k in range(unit):
                src.append(u * unit + k)
                hw.append((y * merge, x * merge) if mutant == "hw_without_merge_offset" else (y * merge + k // merge, x * merge + k % merge))
        # the padded window grid: pad = ws - l % ws, a whole extra (empty) window row / column when l divides evenly
        pad = (lambda l: (ws - l % ws) % ws) if mutant == "no_empty_extra_window" else (lambda l: ws - l % ws)
        nh, nw = (lh + pad(lh)) // ws, (lw + pad(lw)) // ws
        count = {}
        for y, x in units:
            count[(y // ws, x // ws)] = count.get((y // ws, x // ws), 0) + unit
        order = [(b, a) for a in range(nw) for b in range(nh)] if mutant == "column_major_windows" else [(b, a) for b in range(nh) for a in range(nw)]
        row = row_img
        for wkey in order:
            n = count.get(wkey, 0)
            items_win += [(row, n, q, 0) for q in range(-(-n // chunk))]
            max_seg = max(max_seg, n)
            row += n
            cu_raw.append(row)
        n = len(src) - row_img
        items_full += [(row_img, n, q, 0) for q in range(-(-n // chunk))]
        max_seg = max(max_seg, n)
        mbase += lh * lw
    i32 = lambda a, shape: np.array(a, np.int64).reshape(shape)
    return types.SimpleNamespace(src=i32(src, (-1,)), hw=i32(hw, (-1, 2)), slot2row=i32([slot2row[i] for i in range(mbase)], (-1,)),
                                 items_win=i32(items_win, (-1, 4)), items_full=i32(items_full, (-1, 4)), imgs=i32(imgs, (-1, 4)),
                                 counts=(len(src), len(items_win), len(items_full), max_seg), cu=np.unique(i32(cu_raw, (-1,))))


QWEN_MERGE, QWEN_WS, QWEN_WINDOW, QWEN_PATCH = 2, 4, 112, 14
QWEN_SIDES = (1, 3, 4, 5, 8, 9)                                    # merged sides: below, at, above and twice the window side of 4


def qwen_fixture_cases():
    """name -> [(gh, gw)] in patches: one image of every merged size QWEN_SIDES x QWEN_SIDES, then three lists of two or three images."""
    out = {f"{a}x{b}": [(2 * a, 2 * b)] for a in QWEN_SIDES for b in QWEN_SIDES}
    out["two"] = [(6, 10), (8, 8)]
    out["two_wide_tall"] = [(2, 18), (16, 4)]
    out["three"] = [(10, 6), (2, 2), (8, 18)]
    return out


def qwen_sweep():
    """The 338 grid lists: every single image with merged sides 1..13, and 169 pairs."""
    grids = [(2 * a, 2 * b) for a in range(1, 14) for b in range(1, 14)]
    return [[g] for g in grids] + [[grids[i], grids[(7 * i + 3) % len(grids)]] for i in range(len(grids))]


def plan_outputs(p):
    """What a comparison of two window plans looks at."""
    return (p.src, p.hw, p.slot2row, p.items_win, p.items_full, p.imgs, np.array(p.counts))


# ---------------------------------------------------------------------------------------------------------------------------------------
# im2col
# ---------------------------------------------------------------------------------------------------------------------------------------
IM2COL_GEOM = ((6, 2), (12, 3), (28, 14), (42, 14))
CROP_SRC = {1: (2,), 5: (3, 0, 3, 6, 1)}                          # skips, repeats, not monotone; 3 / 7 source crops


def im2col_cases():
    """(img, patch, Kpad, pixel type, ncrop): Kpad = K, K rounded up to 8 and to 64; g * Kpad is below 256 for (6, 2) and (12, 3) with the
    two smaller paddings and at or above it elsewhere (the thread loop strides by 256); both ncrop meet every geometry and pixel type."""
    out = []
    for i, (img, patch) in enumerate(IM2COL_GEOM):
        K = 3 * patch * patch
        for j, Kpad in enumerate((K, -(-K // 8) * 8, -(-K // 64) * 64)):
            for k, pt in enumerate(("f32", "bf16")):
                out.append((img, patch, Kpad, pt, 5 if (i + j + k) % 2 else 1))
        out += [(img, patch, K, "f32", 5), (img, patch, -(-K // 8) * 8, "bf16", 1 if i % 2 else 5)]
    return out


def make_im2col(case):
    img, patch, Kpad, pt, ncrop = case
    nsrc = max(CROP_SRC[ncrop]) + 1
    g = torch.Generator().manual_seed(img * 100 + patch + Kpad + ncrop)
    pix = torch.randn(nsrc, 3, img, img, generator=g)
    pix[0, 0, 0, :2] = torch.tensor([7.0e4, -3.0e-7])              # beyond f16's range, below its subnormals
    if pt == "bf16":
        pix = pix.bfloat16()
    return types.SimpleNamespace(img=img, patch=patch, Kpad=Kpad, pt=pt, ncrop=ncrop, pix=pix, crop_src=np.array(CROP_SRC[ncrop], np.int32),
                                 g=img // patch, K=3 * patch * patch)


def im2col_ref(P, dt, prec, mutant=None):
    """[ncrop g g, Kpad << prec] in the operand type: Conv2d(3, H, k = p, s = p) unfolded; row (crop, py, px), column c p p + ky p + kx."""
    p, rows = P.patch, []
    for c, s in enumerate(P.crop_src):
        x = P.pix[c if mutant == "crop_src_ignored" else int(s)].float()
        cols = torch.nn.functional.unfold(x[None], kernel_size=p, stride=p)[0].t()      # [g g, 3 p p]
        if mutant == "ky_kx_swapped":
            cols = cols.reshape(-1, 3, p, p).transpose(2, 3).reshape(-1, P.K)
        elif mutant == "channel_minor_k":
            cols = cols.reshape(-1, 3, p, p).permute(0, 2, 3, 1).reshape(-1, P.K)
        rows.append(cols)
    v = torch.cat(rows)
    v = torch.cat([v, torch.full((v.shape[0], P.Kpad - P.K), 1.0 if mutant == "pad_not_zero" else 0.0)], dim=1)
    return _encode(v, dt, prec, mutant)


# ---------------------------------------------------------------------------------------------------------------------------------------
# clip_embed
# ---------------------------------------------------------------------------------------------------------------------------------------
CLIP_EMBED_H, CLIP_EMBED_T, CLIP_EMBED_NCROP = (4, 64, 260, 1024, 4096), (5, 17), 3


def clip_embed_cases():
    return [(H, T) for H in CLIP_EMBED_H for T in CLIP_EMBED_T]


def make_clip_embed(case):
    H, T = case
    n = CLIP_EMBED_NCROP
    g = torch.Generator().manual_seed(H * 31 + T)
    r = lambda *s: torch.randn(*s, generator=g)
    return types.SimpleNamespace(H=H, T=T, ncrop=n, patch_out=r(n * (T - 1), H), cls=r(H), pos=0.5 * r(T, H), w=1 + 0.1 * r(H), b=0.1 * r(H),
                                 eps=f32(1e-5))


def clip_embed_run(P, dtype, mutant=None):
    """(y, e) [ncrop T, H] in dtype: CLIPVisionEmbeddings + pre_layrnorm in the kernel's order, and (fp64) the bound of the module docstring.
    Row (crop, t) = LayerNorm((t == 0 ? cls : patch_out[crop (T - 1) + t - 1]) + pos[t])."""
    c = lambda t: t.to(dtype)
    T, H, n = P.T, P.H, P.ncrop
    po = c(P.patch_out)
    stride = T if mutant == "crop_stride_T" else T - 1
    idx = (torch.arange(n)[:, None] * stride + torch.arange(T - 1)[None, :]).clamp_max(po.shape[0] - 1)
    tok = torch.cat([c(P.cls).expand(n, 1, H), po[idx]], dim=1)   # [n, T, H]: class embedding in front of every crop's patch rows
    pos = c(P.pos)
    if mutant == "position_t_minus_1":
        pos = torch.roll(pos, 1, dims=0)
    elif mutant == "cls_position_on_every_row":
        pos = pos[:1].expand(T, H)
    v = (tok + pos[None]).reshape(n * T, H)
    e_v = U32 * v.abs()
    s, ch = lane_sum(v, 64, 4, True)
    mean = s / H
    e_mean = (e_v.sum(dim=1) + U32 * ch) / H + U32 * mean.abs()
    a = v - mean[:, None]
    e_a = e_v + e_mean[:, None] + U32 * a.abs()
    sq = a * a
    e_sq = 2 * a.abs() * e_a + e_a * e_a + U32 * sq
    q, ch = lane_sum(sq, 64, 4, True)
    e_q = e_sq.sum(dim=1) + U32 * ch
    var = q / (H - 1 if mutant == "unbiased_variance" else H)
    e_var = e_q / H + U32 * var
    t = var + P.eps
    rstd, e_r = _rsqrt(t, e_var + U32 * t)
    rstd, e_r = rstd[:, None], e_r[:, None]
    p1 = a * rstd
    e1 = rstd.abs() * e_a + a.abs() * e_r + e_a * e_r + U32 * p1.abs()
    w = c(P.w)
    y = p1 * w
    e = w.abs() * e1 + U32 * y.abs()
    y = y + c(P.b)
    e = e + U32 * y.abs()
    return y, e


def clip_embed_naive(P):
    """The module itself in fp64: cat(class, patches) + position_embedding, then nn.LayerNorm."""
    n, T, H = P.ncrop, P.T, P.H
    x = torch.cat([P.cls.double().expand(n, 1, H), P.patch_out.double().view(n, T - 1, H)], dim=1) + P.pos.double()[None]
    return torch.nn.functional.layer_norm(x, (H,), P.w.double(), P.b.double(), P.eps).reshape(n * T, H)


# ---------------------------------------------------------------------------------------------------------------------------------------
# hd_gather
# ---------------------------------------------------------------------------------------------------------------------------------------
HD_G, HD_H = (2, 4, 6), (4, 64, 260)
HD_BATCHES = {1: ((2, 3),), 2: ((1, 2), (3, 1)), 3: ((1, 1), (2, 1), (2, 3))}
HD_GAPS = (2, 0, 1)                                               # unused crops in front of every sample's first crop


def hd_gather_cases():
    return [(g, H, B) for g in HD_G for H in HD_H for B in (1, 2, 3)]


def hd_layout(grids, gaps, g):
    """samples [(hc, wc, crop0, voff)], crops in the buffer, total rows."""
    smp, nc, rows = [], 0, 0
    for (hc, wc), gap in zip(grids, gaps):
        nc += gap
        smp.append((hc, wc, nc, rows))
        nc += hc * wc + 1
        rows += hd_plan_ref(hc, wc, 1, g)[3]
    return smp, nc, rows


def make_hd_gather(case):
    g, H, B = case
    grids = HD_BATCHES[B]
    smp, nc, rows = hd_layout(grids, HD_GAPS, g)
    gen = torch.Generator().manual_seed(g * 1000 + H + B)
    clipx = torch.randn(nc + 1, g * g + 1, H, generator=gen)       # (+ 1: the crop a mutant reads behind the last sample)
    used = torch.zeros(nc + 1, dtype=torch.bool)
    for hc, wc, c0, _ in smp:
        used[c0:c0 + hc * wc + 1] = True
    return types.SimpleNamespace(g=g, H=H, B=B, T=g * g + 1, samples=np.array(smp, np.int32), ncrops=nc, rows=rows, clipx=clipx, used=used,
                                 sub_gn=torch.randn(4 * H, generator=gen), glb_gn=torch.randn(4 * H, generator=gen))


def _merge2x2(x, g, swapped=False):
    """reshape_hd_patches_2x2merge for N crops x [N, g g, C]: [N, g/2, g/2, 4 C], the 2 x 2 neighbourhood concatenated as (di, dj, channel)."""
    N, _, C = x.shape
    order = (0, 1, 3, 4, 2, 5) if swapped else (0, 1, 3, 2, 4, 5)
    return x.reshape(N, g // 2, 2, g // 2, 2, C).permute(*order).reshape(N, g // 2, g // 2, 4 * C)


def _newline(x, sep, first=False):
    """add_image_newline: x [h, w, C] -> [h (w + 1), C] with sep behind (first: in front of) every row."""
    s = sep.reshape(1, 1, -1).expand(x.shape[0], 1, -1)
    return torch.cat([s, x] if first else [x, s], dim=1).reshape(-1, x.shape[-1])


def hd_gather_values(clipx, samples, g, sub_gn, glb_gn, mutant=None):
    """fp32 [rows, 4 H]: per sample [sub crops merged and laid out hc x wc, newline per row | glb_GN | global crop, newline per row]
    (hd_feature_transform, 'sub_glb').  clipx [crops, g g + 1, H]: token 0 is CLS."""
    g2 = g // 2
    feat = clipx[:, :g * g] if mutant == "cls_not_skipped" else clipx[:, 1:]
    out = []
    for hc, wc, crop0, _ in np.asarray(samples).tolist():
        n = hc * wc
        glb = _merge2x2(feat[crop0 + (1 if mutant == "global_crop_from_crop0_plus_1" else 0)][None], g, mutant == "di_dj_swapped")[0]
        sub = feat[crop0 + 1:crop0 + 1 + n]
        if mutant == "crop_index_hc_for_wc":
            sub = sub[[(i * hc + j) % n for i in range(hc) for j in range(wc)]]
        sub = _merge2x2(sub, g, mutant == "di_dj_swapped").reshape(hc, wc, g2, g2, -1).permute(0, 2, 1, 3, 4).reshape(hc * g2, wc * g2, -1)
        first = mutant == "sub_separator_at_column_0"
        parts = [_newline(sub, sub_gn, first), glb_gn.reshape(1, -1), _newline(glb, sub_gn, first)]
        if mutant == "global_separator_one_row_early":
            parts = [parts[0][:-1], parts[1], parts[0][-1:], parts[2]]
        out += parts
    return torch.cat(out)


def hd_gather_ref(P, dt, prec, mutant=None):
    return _encode(hd_gather_values(P.clipx, P.samples, P.g, P.sub_gn, P.glb_gn, mutant), dt, prec)


# ---------------------------------------------------------------------------------------------------------------------------------------
# clip_tokens
# ---------------------------------------------------------------------------------------------------------------------------------------
def clip_tokens_cases():
    return [(T, H, n) for T in (2, 5, 17) for H in (4, 260) for n in (1, 3)]


def make_clip_tokens(case):
    T, H, n = case
    return types.SimpleNamespace(T=T, H=H, ncrop=n, clipx=torch.randn(n, T, H, generator=torch.Generator().manual_seed(T * 10 + H + n)))


def clip_tokens_ref(P, dt, prec, mutant=None):
    x = P.clipx[:, :P.T - 1] if mutant == "cls_kept" else P.clipx[:, 1:]
    return _encode(x.reshape(-1, P.H), dt, prec)


# ---------------------------------------------------------------------------------------------------------------------------------------
# llava_pack
# ---------------------------------------------------------------------------------------------------------------------------------------
LLAVA_G, LLAVA_D = (2, 4), (4, 64, 260)
LLAVA_GAPS = (1, 0, 2)


def llava_pack_sizes(crop):
    """B -> [(h, w)] at crop size `crop`: B = 1 rows unpadded (r0 > 0); B = 2 rows unpadded by one (a kept height of 2 mod 4 at g = 4: a
    total that is no multiple of 4), a one-column grid;
    B = 3 pad = 0, the strip whose unpad leaves no rows, a one-pixel image (gw = 2, the kept columns straddle the two crops)."""
    c = crop
    return {1: [(c + c // 3, 2 * c + c // 2)], 2: [(8 * c // 5, 2 * c), (5 * c, c // 2)], 3: [(2 * c, c), (1, 2000), (1, 1)]}


LLAVA_HAND_SAMPLE = lambda g: (1, 2, 0, g, g + g // 2, 2 * g)        # gw = 2, c0 inside the second crop, columns kept: no plan yields it; the kernel must still serve it


def llava_pack_cases():
    return [(g, D, B) for g in LLAVA_G for D in LLAVA_D for B in (1, 2, 3)]


def llava_layout(geoms, gaps, g):
    """geoms [(gh, gw, r0, r1, c0, c1)] -> samples [(.., crop0, voff)], crops in the buffer, total rows."""
    smp, nc, rows = [], 0, 0
    for (gh, gw, r0, r1, c0, c1), gap in zip(geoms, gaps):
        nc += gap
        smp.append((gh, gw, r0, r1, c0, c1, nc, rows))
        nc += 1 + gh * gw
        rows += g * g + (r1 - r0) * (c1 - c0 + 1)
    return smp, nc, rows


def make_llava_pack(case, geoms=None):
    """geoms: the per-sample geometry (the GPU test passes what the plan entry returned); default: the reference plan's.  B = 3 gets the
    hand-made sample as a fourth."""
    g, D, B = case
    crop = 14 * g
    if geoms is None:
        geoms = [llava_plan_ref(h, w, pinpoints(crop), crop, g)[:6] for h, w in llava_pack_sizes(crop)[B]]
    geoms = [tuple(int(v) for v in x) for x in geoms]
    if B == 3:
        geoms = geoms + [LLAVA_HAND_SAMPLE(g)]
    smp, nc, rows = llava_layout(geoms, LLAVA_GAPS + (1,), g)
    gen = torch.Generator().manual_seed(g * 1000 + D + B)
    return types.SimpleNamespace(g=g, D=D, B=len(smp), samples=np.array(smp, np.int32), ncrops=nc, rows=rows,
                                 proj=torch.randn(nc + 1, g * g, D, generator=gen), newline=torch.randn(D, generator=gen))


def llava_pack_ref(proj, samples, g, newline, mutant=None):
    """fp32 [rows, D]: per sample [base crop | rows r0..r1, columns c0..c1 of the (gh g) x (gw g) grid of crops, newline behind every row]
    (pack_image_features + unpad_image as slices).  proj [crops, g g, D]."""
    D = proj.shape[-1]
    out = []
    for gh, gw, r0, r1, c0, c1, crop0, _ in np.asarray(samples).tolist():
        n = gh * gw
        out.append(proj[crop0 + (1 if mutant == "base_crop_from_crop0_plus_1" else 0)])
        tiles = proj[crop0 + 1:crop0 + 1 + n]
        if mutant == "crop_index_gh_for_gw":
            tiles = tiles[[(i * gh + j) % n for i in range(gh) for j in range(gw)]]
        tiles = tiles.reshape(gh, gw, g, g, D)
        if mutant == "y_x_in_crop_swapped":
            tiles = tiles.transpose(2, 3)
        grid = tiles.permute(0, 2, 1, 3, 4).reshape(gh * g, gw * g, D)
        if mutant == "r0_used_for_columns":
            kept = grid[r0:r1, r0:r0 + (c1 - c0)]
            kept = torch.cat([kept, grid[r0:r1, :c1 - c0 - kept.shape[1]]], dim=1)      # (wraps where r0 + width runs off the grid)
        else:
            kept = grid[r0:r1, c0:c1]
        out.append(_newline(kept, newline, mutant == "newline_before_row"))
    return torch.cat(out)


# ---------------------------------------------------------------------------------------------------------------------------------------
# qwen_patch_gather
# ---------------------------------------------------------------------------------------------------------------------------------------
QWEN_GATHER_GRID, QWEN_GATHER_AT = [(6, 10), (4, 6)], 20            # rows src[20 : 20 + rows] of this plan: inside the second window, no identity stretch


def qwen_gather_cases():
    return [(K, Kpad, rows, pt) for K, Kpad in ((1176, 1176), (1176, 1216), (12, 16)) for rows in (1, 37) for pt in ("f32", "bf16")]


def make_qwen_gather(case, src=None):
    """src: the whole src table of QWEN_GATHER_GRID (the GPU test passes the plan entry's); default: the reference plan's."""
    K, Kpad, rows, pt = case
    if src is None:
        src = qwen_window_plan_ref(QWEN_GATHER_GRID, QWEN_MERGE, QWEN_WS).src
    npatch = sum(a * b for a, b in QWEN_GATHER_GRID)
    pix = torch.randn(npatch, K, generator=torch.Generator().manual_seed(K + Kpad + rows))
    pix[0, 0], pix[-1, -1] = 7.0e4, -3.0e-7
    if pt == "bf16":
        pix = pix.bfloat16()
    return types.SimpleNamespace(K=K, Kpad=Kpad, rows=rows, pt=pt, pix=pix, src=np.asarray(src[QWEN_GATHER_AT:QWEN_GATHER_AT + rows], np.int32))


def qwen_gather_ref(P, dt, prec, mutant=None):
    pix = P.pix
    if mutant == "bf16_read_as_fp16" and P.pt == "bf16":
        pix = pix.view(torch.int16).view(torch.float16)
    idx = torch.arange(P.rows) if mutant == "identity_order" else torch.from_numpy(P.src.astype(np.int64))
    v = pix.float()[idx]
    v = torch.cat([v, torch.full((P.rows, P.Kpad - P.K), 1.0 if mutant == "pad_not_zero" else 0.0)], dim=1)
    return _encode(v, dt, prec)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the host entries through ctypes (host only: they run without a device)
# ---------------------------------------------------------------------------------------------------------------------------------------
def lib_sample_plan(lib, backbone, crop, g, pins, h, w):
    """lr_vision_sample_plan: (rc, sample ints, crops, rows)."""
    import ctypes as C
    n = len(pins) if pins else 0
    pin = (C.c_int32 * max(2 * n, 1))(*[v for p in (pins or []) for v in p])
    smp, nc, nr = (C.c_int32 * 8)(*([-7] * 8)), C.c_int32(-7), C.c_int32(-7)
    rc = lib.lr_vision_sample_plan(backbone, crop, g, pin if n else None, n, h, w, smp, C.byref(nc), C.byref(nr))
    return rc, list(smp)[:4 if backbone == LR_BACKBONE_PHI3V else 8], nc.value, nr.value


def lib_qwen_plan(lib, grids, merge=QWEN_MERGE, window=QWEN_WINDOW, patch=QWEN_PATCH, capacity=None):
    """lr_qwen_vision_plan -> (rc, namespace like qwen_window_plan_ref's, without cu).  Every array is allocated at its documented
    capacity with a sentinel behind the part the plan may write."""
    import ctypes as C
    n, unit = len(grids), max(merge * merge, 1)
    P = sum(a * b for a, b in grids) if capacity is None else capacity
    thw = (C.c_int64 * (3 * n))(*[v for a, b in grids for v in (1, a, b)])
    S = -77
    caps = dict(src=P, hw=2 * P, slot2row=P // unit, items_win=4 * (P // unit), items_full=4 * (P // 128 + n), imgs=4 * n, counts=4)
    buf = {k: np.full(v + 4, S, np.int32) for k, v in caps.items()}
    ptr = lambda k: buf[k].ctypes.data_as(C.POINTER(C.c_int32))
    rc = lib.lr_qwen_vision_plan(thw, n, merge, window, patch, P, ptr("src"), ptr("hw"), ptr("slot2row"), ptr("items_win"), ptr("items_full"),
                                 ptr("imgs"), ptr("counts"))
    if rc != 0:
        assert all(bool((b == S).all()) for b in buf.values()), "a refused plan wrote"
        return rc, None
    N, nwin, nfull, max_seg = (int(v) for v in buf["counts"][:4])
    used = dict(src=N, hw=2 * N, slot2row=N // unit, items_win=4 * nwin, items_full=4 * nfull, imgs=4 * n, counts=4)
    for k, b in buf.items():
        assert used[k] <= caps[k] and bool((b[used[k]:] == S).all()), f"{k}: written past its {used[k]} entries"
    a = lambda k, shape: buf[k][:used[k]].astype(np.int64).reshape(shape)
    return rc, types.SimpleNamespace(src=a("src", (-1,)), hw=a("hw", (-1, 2)), slot2row=a("slot2row", (-1,)), items_win=a("items_win", (-1, 4)),
                                     items_full=a("items_full", (-1, 4)), imgs=a("imgs", (-1, 4)), counts=(N, nwin, nfull, max_seg))
