"""fp64 reference, per-element error bound, input families, reference mutants and the dispatch table of the attention kernels
(csrc/attention.hip), for tests/test_attention_reference.py (CPU) and tests/test_gpu_attention.py (MI355X).

Contract of the reference (what attn_kernel computes):
  * key j is visible to query i when mask[j] != 0, j <= i (causal launches), and i, j lie in the same segment (ragged launches);
  * a row with at least one visible key is the softmax over its visible keys of scale * q.k, times V;
  * a row with no visible key is exact zeros (the kernel's epilogue: inv = l_run > 0 ? 1 / l_run : 0);
  * GQA: query head h reads key / value head h // kv_group (repeat_interleave).

Error bound (reference(), second result): derived from the kernel's rounding points, per output element (i, d).  u = unit roundoff of the operand type
(bf16 2^-8, f16 2^-11), u32 = 2^-24, P = the exact normalised weights, o = the exact output, nt = 64-key tiles of the row's sequence.
  Scores.  S^T = K Q^T on 32x32x16 MFMAs accumulating in fp32: HD / 16 steps per contraction (three contractions in split form), at
  most 5 roundings per step (a 16-term MFMA sum) -> |ds| <= (5 nsteps + 2) u32 scale (|Q||K|^T).  Split form drops lo.lo: + scale
  (|Q_lo||K_lo|^T).  In log2 units (x log2 e) the argument fma(s, sc, -m) rounds once (u32 |a|, a <= lazy_t relative to the running
  reference), the rescale chain adds one rounded subtraction per rise of the reference (<= u32 2M, M = max |s sc| of the row) and
  one exp2 per rescale (2 u32 each, <= nt of them).  A relative error eps_ij of the weight w_ij moves o_i by
  sum_j P_ij eps_ij (|v_j| + |o_i|): E_w = (P o eps) |V| + (P o eps) 1 |o|.
  Single pass.  P is rounded to the operand type against the fp32 denominator: u (P |V|); f16 weights below 2^-14 (relative to the
  running reference; a superset: the final weights below 2^-14) are subnormal, absolute error 2^-25 each: 2^-25 (w_small |V|) / l.
  PV accumulates in fp32 over 2 ceil(S / 16) roundings + one per rescale: g_acc (P |V|).  The denominator: 32 sums per lane, one
  exchange, one add and one rescale per tile: g_l = (34 + 2 nt) u32 on |o|.  O = o * (1 / l) (3 u32) is rounded to the operand type
  once: u |o| (+ 2^-25 absolute in f16).
  Split form (hi + lo operands, hi.hi + hi.lo + lo.hi).  P = P_hi + P_lo leaves u^2 P; P_lo . V_lo is dropped: u (P |V_lo|); f16 P_lo is
  subnormal for weights below 2^-3: 2^-25 (w |V|) / l over all visible keys.  O leaves as O_hi + O_lo: u^2 |o| (+ 2^-25 in f16).  PV
  takes three MFMAs per step: g_acc = (6 ceil(S / 16) + nt + 2) u32.  bf16 and f16 thus differ by u^2 = 2^-16 against 2^-22.
The bound is a worst case over rounding errors (every rounding at its maximum, with one sign); the observed err / bound is printed by
the GPU tests.
"""
import math
import re

import torch

LOG2E = 1.4426950408889634
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
U32 = 2.0 ** -24
F16_SUB = 2.0 ** -25          # half the smallest f16 subnormal: absolute rounding error below 2^-14
F16_MIN_NORMAL = 2.0 ** -14
KT = 64                       # keys per tile
ATT_MAX_S = 8192
POISON_V = 3.0e4              # |v| of poisoned (masked) keys: finite in f16 and bf16

MUTANTS = ("drop_key", "diag_plus1", "diag_minus1", "drop_last_tile", "kmin_round_up", "unmask_one", "wave_causal")
FAMILIES = ("normal", "ramp", "poison")


# ---------------------------------------------------------------------------------------------------------------------------------------
# dispatch table of launch_one, as data
# ---------------------------------------------------------------------------------------------------------------------------------------
FORMS = ((96, True), (64, False), (64, True), (96, False), (128, True))        # launch_attention's (head_dim, causal) forms
BANDS = ("single<1024", "single>=1024", "split<=128", "split<1024", "split>=1024")
# (PREC, NW, PP) per band and form, in FORMS order (the table of the issue that opened this suite)
TABLE = {
    "single<1024": [(False, 4, False)] * 5,
    "single>=1024": [(False, 8, True)] * 5,
    "split<=128": [(True, 4, False)] * 5,
    "split<1024": [(True, 8, False), (True, 4, False), (True, 4, False), (True, 8, False), (True, 8, False)],
    "split>=1024": [(True, 8, True)] * 4 + [(True, 8, False)],
}
RAGGED = {(64, False): [(False, 4, False), (True, 4, False)], (96, False): [(False, 4, False), (True, 4, False)]}
PP_MIN_S = 1024


def dispatch(hd, causal, split, S, pingpong=True, ragged=False):
    """(PREC, NW, PP) of the attn_kernel instantiation launch_one picks (LR_ATT_PP_MIN_S at its default)."""
    if (hd, causal) not in FORMS:
        raise ValueError("no such attention form")
    if ragged and causal:
        raise ValueError("ragged mode is dense")
    if not split and not ragged and S >= PP_MIN_S and pingpong:
        return (False, 8, True)
    if split and not ragged and S >= PP_MIN_S and hd != 128 and pingpong:
        return (True, 8, True)
    if split and not ragged and hd == 64 and S > 128:
        return (True, 4, False)
    if split and not ragged and S > 128:
        return (True, 8, False)
    return (split, 4, False)


def band(split, S):
    if not split:
        return "single<1024" if S < PP_MIN_S else "single>=1024"
    return "split<=128" if S <= 128 else "split<1024" if S < PP_MIN_S else "split>=1024"


def all_cells():
    """Every (hd, causal, PREC, NW, PP, ragged) launch_one can reach, from TABLE and RAGGED."""
    cells = set()
    for bd, row in TABLE.items():
        for (hd, causal), inst in zip(FORMS, row):
            cells.add((hd, causal) + inst + (False,))
    for (hd, causal), insts in RAGGED.items():
        for inst in insts:
            cells.add((hd, causal) + inst + (True,))
    return cells


def launch_sites(src):
    """(PREC, NW, PP) of every attn_kernel launch in launch_one's source text."""
    body = src[src.index("static void launch_one"):src.index("void launch_attention")]
    out = set()
    for m in re.finditer(r"attn_kernel<OT, HD, CAUSAL, (true|false), (4|8)(?:, (true|false))?>", body):
        out.add((m.group(1) == "true", int(m.group(2)), m.group(3) == "true"))
    return out


def attention_forms(src):
    """(head_dim, causal) pairs launch_attention dispatches, from its source text."""
    body = src[src.index("void launch_attention"):]
    return {(int(h), c == "") for h, c in re.findall(r"head_dim == (\d+) && (!?)causal", body)}


# ---------------------------------------------------------------------------------------------------------------------------------------
# visibility
# ---------------------------------------------------------------------------------------------------------------------------------------
def kmin_of(mask_row):
    """First valid key of a mask row (S when there is none): what the engine passes as kmin."""
    nz = torch.nonzero(mask_row != 0)
    return int(nz[0]) if len(nz) else int(mask_row.numel())


def visible(qi, S, causal, mask_row=None, seg=None, mutant=None):
    """bool [len(qi), S]: key j visible to query qi[r].  seg: int [S] segment id of each row (ragged mode), else None.
    mutant: one of MUTANTS (a deliberately wrong rule, for the tests of the bound's power) or None."""
    dev = qi.device
    j = torch.arange(S, device=dev)
    ok = torch.ones(len(qi), S, dtype=torch.bool, device=dev)
    mk = (mask_row != 0) if mask_row is not None else torch.ones(S, dtype=torch.bool, device=dev)
    if mutant == "unmask_one" and mask_row is not None and not bool(mk.all()):
        mk = mk.clone()
        mk[int(torch.nonzero(~mk)[-1])] = True          # the LAST masked key (left padding: the one next to the first valid key)
    ok &= mk[None, :]
    if causal:
        lim = qi
        if mutant == "diag_plus1":
            lim = qi + 1
        elif mutant == "diag_minus1":
            lim = qi - 1
        elif mutant == "wave_causal":
            lim = (qi // 32) * 32 + 31                  # the causal limit of a 32-query wave (its last query) for every query of it
        ok &= j[None, :] <= lim[:, None]
    if seg is not None:
        ok &= seg[qi][:, None] == seg[None, :]
        start = torch.zeros_like(seg)
        start[1:] = torch.where(seg[1:] != seg[:-1], torch.arange(1, S, device=dev), torch.zeros_like(seg[1:]))
        start = torch.cummax(start, 0).values          # first row of each row's segment
    else:
        start = torch.zeros(S, dtype=torch.long, device=dev)
    if mutant == "drop_last_tile":
        if seg is None:
            ok &= j[None, :] < ((S - 1) // KT) * KT
        else:
            end = torch.zeros(S, dtype=torch.long, device=dev)
            for s in torch.unique(seg).tolist():
                rows = torch.nonzero(seg == s).flatten()
                end[rows] = int(rows[-1]) + 1
            ok &= (j - start)[None, :] < (((end - start - 1) // KT) * KT)[None, :]
    if mutant == "kmin_round_up" and causal and mask_row is not None:
        km = kmin_of(mask_row)
        ok &= j[None, :] >= -(-km // KT) * KT
    if mutant == "drop_key":
        last = torch.where(ok, j[None, :], torch.full_like(ok, -1, dtype=torch.long)).max(dim=1).values
        rows = torch.nonzero(last >= 0).flatten()
        ok[rows, last[rows]] = False
    return ok


# ---------------------------------------------------------------------------------------------------------------------------------------
# reference and bound
# ---------------------------------------------------------------------------------------------------------------------------------------
def reference(q, k, v, *, scale, causal, mask=None, segments=None, kv_group=1, dtype="bf16", split=False, lo=None, lazy_t=0.0,
              mutant=None, want_bound=True, chunk=256):
    """q [B, S, H, HD], k / v [B, S, Hkv, HD]: the values the kernel is given, as fp64 (split form: hi + lo).  lo = (q_lo, k_lo, v_lo)
    residual halves (split form only, for the dropped lo.lo terms).  mask: [B, S] or None.  segments: cu_seqlens (list, ragged
    mode, B = 1).  Returns (o, bound) as fp64 [B, S, H, HD] (bound None when want_bound is False), computed in query chunks."""
    B, S, H, HD = q.shape
    dev = q.device
    q, k, v = q.double(), k.double(), v.double()
    seg = None
    if segments is not None:
        seg = torch.zeros(S, dtype=torch.long, device=dev)
        for i, (a, b) in enumerate(zip(segments[:-1], segments[1:])):
            seg[a:b] = i
    o = torch.zeros(B, S, H, HD, dtype=torch.float64, device=dev)
    bnd = torch.zeros_like(o) if want_bound else None
    u = U[dtype]
    if want_bound:
        ql, kl, vl = (x.double() for x in lo) if split else (None, None, None)
        nsteps = (HD // 16) * (3 if split else 1)
        c_acc_s = (5 * nsteps + 2) * U32
    for b in range(B):
        mrow = mask[b] if mask is not None else None
        seglen = None
        if seg is not None:                                 # per-row length of its segment (tiles, fp32 sums)
            cnt = torch.bincount(seg, minlength=len(segments) - 1)
            seglen = cnt[seg].double()
        for h in range(H):
            kh = h // kv_group
            K, V = k[b, :, kh], v[b, :, kh]
            Va = V.abs()
            for c0 in range(0, S, chunk):
                c1 = min(S, c0 + chunk)
                qi = torch.arange(c0, c1, device=dev)
                ok = visible(qi, S, causal, mrow, seg, mutant)
                s = (q[b, c0:c1, h] @ K.T) * scale
                sm = s.masked_fill(~ok, float("-inf"))
                mx = sm.max(dim=1, keepdim=True).values
                any_ok = ok.any(dim=1, keepdim=True)
                mx = torch.where(any_ok, mx, torch.zeros_like(mx))
                w = torch.exp(sm - mx) * ok
                l = w.sum(dim=1, keepdim=True)
                linv = torch.where(any_ok, 1.0 / torch.where(any_ok, l, torch.ones_like(l)), torch.zeros_like(l))
                P = w * linv
                oc = P @ V
                o[b, c0:c1, h] = oc
                if not want_bound:
                    continue
                n = seglen[c0:c1, None] if seglen is not None else torch.full((c1 - c0, 1), float(S), dtype=torch.float64, device=dev)
                nt = torch.ceil(n / KT)
                a = (s - mx) * LOG2E                                              # log2 weight (<= 0 at the row maximum)
                absqk = (q[b, c0:c1, h].abs() @ K.abs().T) * scale * LOG2E
                da = c_acc_s * absqk + U32 * (a.abs() + lazy_t)
                if split:
                    da = da + (ql[b, c0:c1, h].abs() @ kl[b, :, kh].abs().T) * scale * LOG2E
                M = (s * LOG2E).abs().masked_fill(~ok, 0).max(dim=1, keepdim=True).values
                da = da + 2 * U32 * M
                eps = math.log(2.0) * da + (2 + 2 * nt) * U32
                Pe = P * eps
                oa = oc.abs()
                PV = P @ Va
                E = Pe @ Va + Pe.sum(dim=1, keepdim=True) * oa
                g_l = (34 + 2 * nt) * U32
                if not split:
                    g_acc = (2 * torch.ceil(n / 16) + nt + 2) * U32
                    bb = (u + g_acc) * PV + E + (u + g_l + 3 * U32) * oa
                    if dtype == "f16":
                        small = ((w < F16_MIN_NORMAL) & ok).double() * linv
                        bb = bb + F16_SUB * (small @ Va) + F16_SUB
                else:
                    g_acc = (6 * torch.ceil(n / 16) + nt + 2) * U32
                    bb = (u * u + g_acc) * PV + u * (P @ vl[b, :, kh].abs()) + E + (u * u + g_l + 3 * U32) * oa
                    if dtype == "f16":
                        bb = bb + F16_SUB * ((ok.double() * linv) @ Va) + F16_SUB
                bnd[b, c0:c1, h] = torch.where(any_ok, bb, torch.zeros_like(bb))
    return o, bnd


def naive(q, k, v, *, scale, causal, mask=None, segments=None, kv_group=1):
    """The whole S x S softmax at once in fp64 (for checking reference() on small shapes)."""
    B, S, H, HD = q.shape
    kk = k.double().repeat_interleave(kv_group, dim=2).permute(0, 2, 1, 3)
    vv = v.double().repeat_interleave(kv_group, dim=2).permute(0, 2, 1, 3)
    s = q.double().permute(0, 2, 1, 3) @ kk.transpose(2, 3) * scale
    ok = torch.ones(B, 1, S, S, dtype=torch.bool, device=q.device)
    if causal:
        ok = ok & torch.tril(torch.ones(S, S, dtype=torch.bool, device=q.device))
    if mask is not None:
        ok = ok & (mask != 0)[:, None, None, :]
    if segments is not None:
        seg = torch.zeros(S, dtype=torch.long, device=q.device)
        for i, (a, b) in enumerate(zip(segments[:-1], segments[1:])):
            seg[a:b] = i
        ok = ok & (seg[:, None] == seg[None, :])
    p = torch.softmax(s.masked_fill(~ok, float("-inf")), dim=-1).nan_to_num(0.0)
    return (p @ vv).permute(0, 2, 1, 3)


def max_ratio(err, bound):
    """max(err / bound) over the elements (0 / 0 counts as 0: rows with no visible key must be exact zeros)."""
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return r.max().item()


# ---------------------------------------------------------------------------------------------------------------------------------------
# input families
# ---------------------------------------------------------------------------------------------------------------------------------------
def _carrier_c(scale, slope=0.5):
    """Power of two c with c * scale * log2 e close to `slope` log2 units per key (exact in both operand types)."""
    return 2.0 ** round(math.log2(slope / (scale * LOG2E)))


def make_inputs(family, B, S, H, Hkv, HD, *, scale, mask=None, segments=None, sigma=1.0, seed=0, device="cpu"):
    """fp32 q [B, S, H, HD], k / v [B, S, Hkv, HD] of one input family (before rounding to the operand type).
    normal: N(0, sigma).  ramp: three carrier coordinates make the score rise by ~0.5 log2 units per key (q = (64c, c, -64c t_i),
    k = (t_j, r_j, 1) with j = 64 t_j + r_j, i's tile t_i: exact in both operand types, the row-constant part cancels in the softmax),
    so the latest visible key of every row dominates it and a one-key fault at the causal edge or in the last tile is large; masked
    keys score high as in poison (their values stay N(0, sigma)).
    poison: masked-out keys (ragged: keys of the neighbouring segments) score ~40 log2 units above every visible key and carry
    |v| = 3e4; a leaked key is orders of magnitude over the bound.  Ragged positions count from the start of each segment."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randn(B, S, H, HD, generator=g) * sigma
    k = torch.randn(B, S, Hkv, HD, generator=g) * sigma
    v = torch.randn(B, S, Hkv, HD, generator=g) * sigma
    pos = torch.arange(S)
    seg = torch.zeros(S, dtype=torch.long)
    if segments is not None:
        for i, (a, b) in enumerate(zip(segments[:-1], segments[1:])):
            seg[a:b] = i
            pos[a:b] = torch.arange(b - a)
    if family == "ramp":
        c = _carrier_c(scale)
        q[..., 0] = 64 * c
        q[..., 1] = c
        q[..., 2] = (-64 * c * (pos // KT)).float()[None, :, None]
        k[..., 0] = (pos // KT).float()[None, :, None]
        k[..., 1] = (pos % KT).float()[None, :, None]
        k[..., 2] = 1.0
    elif family != "poison" and family != "normal":
        raise ValueError(family)
    if family in ("ramp", "poison"):
        a_ = 2.0 ** round(math.log2(math.sqrt(40.0 / (scale * LOG2E))))
        if segments is not None:
            par = (seg % 2).float()
            q[..., 3] = (a_ * par)[None, :, None]
            q[..., 4] = (a_ * (1 - par))[None, :, None]
            k[..., 3] = (a_ * (1 - par))[None, :, None]
            k[..., 4] = (a_ * par)[None, :, None]
        elif mask is not None:
            bad = (mask.cpu() == 0).float()                              # [B, S]
            q[..., 3] = a_
            k[..., 3] = (a_ * bad)[:, :, None]
            sign = torch.where(torch.arange(HD) % 2 == 0, 1.0, -1.0)
            if family == "poison":
                v = torch.where((bad != 0)[:, :, None, None], POISON_V * sign, v)
    return q.to(device), k.to(device), v.to(device)


def split(x, tdt):
    """hi = round(x), lo = round(x - hi) in the operand type (csrc/common.h split2)."""
    hi = x.to(tdt)
    return hi, (x - hi.float()).to(tdt)
