"""fp64 reference, per-element error bound, input families, reference mutants and fp32 emulation of the floating-point row kernels:
the norm operand producers (csrc/rowops.hip norm_rows_kernel / norm_rows8_kernel), csrc/gemm_f32.hip and the fp32 reward tail
(gather_norm, rowvec_linear, ca_scores, ca_softmax, ca_context, reward_head, rms_rows_f32, ca_softmax_pad, ca_pool), for
tests/test_rowops_reference.py (CPU) and tests/test_gpu_rowops.py (MI355X).  Built like helpers/gemm_ref.py, whose operand-format
helpers (split, round_op, e8m0_of_amax, qerr, block_E) it reuses.

Contract of the reference: the plain fp64 operation on THE fp32 VALUES THE KERNEL IS GIVEN (eps, scale and alpha after their rounding to
fp32; bf16 B of gemm_f32 as the bf16 values).  Every op is one function run(P, dtype): the operation written in the kernel's own
summation order.  With dtype = float64 it is the reference (equal to the one-line naive() of the op to 1e-12, which the CPU file checks)
and it returns the bound beside the value; with dtype = float32 it is the stand-in for the device on a CPU (emulate()).

Error bound, per output element, from the kernel's rounding points; first order in u32 = 2^-24, u = unit roundoff of the operand type.
hipcc contracts a * b + c into an fma in device code; every product and every sum is charged its own rounding, which holds either way.
  Row sums (lane_sum).  A lane sums its own columns in order (the 4-wide kernels and rowvec_linear / ca_scores first sum the 4 terms of
  a float4, then add that to the lane's accumulator; the 8-wide kernel adds its 8 elements one by one; scalar kernels stride by 64 or
  256), then 6 butterfly steps (wave_sum), then for block kernels the serial sum of the 4 waves (block_reduce).  Charged
  u32 * sum over additions of |S_t|, S_t the fp64 partial sum that addition produces, additions of a zero left out (they are exact);
  plus what the terms carry in (u32 |x y| for a product term).  Not n u32 sum |x|.
  Norms.  mean = s / H one rounding; a = x - mean one rounding + the mean's error; a^2: 2 |a| e_a + e_a^2 + u32 a^2; q by lane_sum;
  q / H + eps two roundings; rsqrtf: propagated through its (convex, decreasing) graph, rsqrt(t - e_t) - rsqrt(t), plus RSQRT_ULP ulp
  = 2 RSQRT_ULP u32 relative (2: OpenCL's limit for rsqrt, which OCML implements; the hardware v_rsq_f32 is documented at 1);
  (a * rstd) * w two roundings, + b one.  RMSNorm: mean = 0 and a = x exactly.  The fp32 tail norms: w * (x * rstd), two roundings.
  Output format of the norms, as gemm_ref charges it: single u |y| (f16: + 2^-25; saturation at 65504, the reference clamps the same
  way); [hi | lo]: u (u |y| + max(0, |y| - 65504)) (f16: + 2^-25); one-byte residual half: q(r, E) = max(2^-4 |r|, 2^-17 max_block |r|)
  on |r| <= u (|y| + e) + max(0, |y| + e - 65504) (f16: + 2^-25), the reference is not clamped in that form.
  Softmax.  r - mx one rounding, through exp: e (u32 |r - mx|); expf 1 ulp = 2 u32 (HIP math API table, as gemm_ref); the sum by
  lane_sum over 256 lanes; an exponential or a probability below 2^-126 may be denormal or flushed (+ 2^-126 absolute); the pad term
  (float)npad * expf(-mx): 2 u32 + one product; 1 / s one rounding; e * inv one rounding.
  gemm_f32.hip.  One chain per element in k order; every 32x32x2 step is charged c(2) = 2 roundings against the partial sum after the
  step plus that step's |a||b| (gemm_ref's convention for an MFMA step of depth d); alpha one more.
  ca_context: four chains (j % 4) of rounded products, the vb % 4 tail into the first, (a0 + a1) + (a2 + a3).
  ca_pool: h + u and + o one rounding each, the squares and their block sum, rstd, w * (v * rstd) two roundings, the running sum over
  the valid tokens one rounding each, 1 / max(cnt, 1e-8) and the final product one each.
The bound is a worst case with every rounding at its maximum and one sign, so it gets no margin factor.  On the `exact` family (small
integers and dyadic fractions, alpha / scale powers of two) every partial sum in any order is exact in fp32: the output must equal the
fp64 reference BIT FOR BIT.
"""
import itertools
import math
import types

import torch

from .gemm_ref import F16_MAX, F16_SUB, POISON, TDT, U, U32, block_E, e8m0_of_amax, max_ratio, qerr, round_op, split  # noqa: F401

RSQRT_ULP = 2                  # rsqrtf: ulp charged (module docstring)
F32_MIN = 2.0 ** -126          # fp32 results below the smallest normal may arrive denormal or flushed: absolute term of the softmax bound
NORM_MAXC = 16                 # csrc/rowops.hip: H <= 4096
F64, F32 = torch.float64, torch.float32

NORM_FAMILIES = ("normal", "offset", "tiny5", "tiny6", "outlier", "zero_row")      # tiny5 / tiny6: |x| ~ 1e-3 under eps 1e-5 / 1e-6
NORM_MUTANTS = ("eps_dropped", "mean_kept_in_output", "bias_dropped", "weight_shift4", "sum_misses_last_chunk", "divides_by_padded_H",
                "lo_zero", "lo_of_unrounded_hi", "group_rows_transposed", "scale_off_by_one", "scale_tile_ignored")
GEMM_MUTANTS = ("drop_last_ktile", "odd_k_lost", "b_transposed", "alpha_dropped", "ld_ignored", "row_clamp_leak", "col_clamp_leak")
TAIL_MUTANTS = {
    "gather_norm": ("gathers_first_valid", "last_valid_off_by_one", "eps_dropped", "weight_shift4"),
    "rms_rows_f32": ("eps_dropped", "weight_shift4", "sum_misses_last_chunk"),
    "rowvec_linear": ("sum_misses_last_chunk", "head_k_reads_row0"),
    "ca_scores": ("pad_scores_read_next_row", "voff_stride_ignored", "scale_dropped", "sum_misses_last_chunk"),
    "ca_softmax": ("no_max_subtraction",),
    "ca_softmax_pad": ("no_max_subtraction", "pad_term_dropped"),
    "ca_context": ("context_tail_dropped", "voff_stride_ignored"),
    "reward_head": ("no_ca_norm", "head_k_reads_row0"),
    "ca_pool": ("pool_counts_pads", "pool_divides_by_S", "pool_u_after_norm"),
}
TAIL_FAMILIES = {
    "gather_norm": ("normal", "tiny5", "outlier", "zero_row"), "rms_rows_f32": ("normal", "tiny6", "outlier", "zero_row"),
    "rowvec_linear": ("normal", "outlier", "exact"), "ca_scores": ("normal", "outlier", "exact"),
    "ca_softmax": ("normal", "ramp_hi"), "ca_softmax_pad": ("normal", "ramp_hi", "all_low"),
    "ca_context": ("normal", "outlier", "exact"), "reward_head": ("normal", "outlier", "tiny5"), "ca_pool": ("normal", "outlier", "tiny5"),
}


def f32(v):
    """A python float after its rounding to fp32 (what a `float` argument of the C entry point holds)."""
    return torch.tensor(v, dtype=F32).item()


def ratio(err, bound):
    """max(err / bound), a NaN or infinite error counting as infinite (a mutant that overflows is caught)."""
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return max_ratio(err, bound) if err.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# the one-byte residual form's scale array (csrc/common.h)
# ---------------------------------------------------------------------------------------------------------------------------------------
def lo8_sidx(r):
    return ((((r >> 6) & 1) * 16 + (r & 15)) * 2 + (r >> 7)) * 4 + ((r >> 4) & 3)


def lo8_scale_at(row, kblock, M):
    """Python port of common.h lo8_scale_at: byte offset of the E8M0 scale of (row, 128-column block) of an operand with M rows."""
    return ((kblock >> 2) * ((M + 255) // 256) + (row >> 8)) * 1024 + (kblock & 3) * 256 + lo8_sidx(row & 255)


def lo8_scale_bytes(M, K):
    return ((M + 255) // 256) * 1024 * ((K // 128 + 3) // 4)


def lo8_scales_decode(scales, M, K):
    """E [M, K / 128] (uint8) out of a scale array in the consuming kernel's lane order: per group of 4 K-tiles and 256-row tile one KB =
    4 slices of 256 bytes, the byte of row r at lo8_sidx(r) of its slice."""
    Mb, nkb = (M + 255) // 256, K // 128
    planes = scales[: Mb * 1024 * ((nkb + 3) // 4)].view((nkb + 3) // 4, Mb, 4, 256).permute(0, 2, 1, 3).reshape(-1, Mb, 256)[:nkb]   # [kblock, Mb, 256]
    r = torch.arange(256, device=scales.device)
    sidx = ((((r >> 6) & 1) * 16 + (r & 15)) * 2 + (r >> 7)) * 4 + ((r >> 4) & 3)
    return planes[:, :, sidx].reshape(nkb, Mb * 256)[:, :M].t()


def lo8_scale_index(M, K, device="cpu", tile_ignored=False):
    """lo8_scale_at of every (row, block) as an index tensor [M, K / 128]."""
    row = torch.arange(M, device=device)[:, None]
    kb = torch.arange(K // 128, device=device)[None, :]
    tile = torch.zeros_like(row) if tile_ignored else row >> 8
    return ((kb >> 2) * ((M + 255) // 256) + tile) * 1024 + (kb & 3) * 256 + lo8_sidx(row & 255)


# ---------------------------------------------------------------------------------------------------------------------------------------
# row sums in the kernels' order
# ---------------------------------------------------------------------------------------------------------------------------------------
def _add(a, b, charge):
    """a + b and the charge |a + b| where neither term is zero (x + 0 is exact), summed per row into charge."""
    s = a + b
    both = (a != 0) & (b != 0)
    c = (s.abs() * both).reshape(s.shape[0], -1).sum(dim=1)
    return s, charge + c


def lane_sum(t, lanes=64, width=1, presum=False):
    """Sum of the rows of t [R, n] in the order of a row kernel, in t's dtype: column e belongs to chunk e // width, chunk c to lane
    c % lanes in sweep c // lanes; presum: the chunk is summed first and then added to the lane's accumulator, else its elements are
    added one by one; then the xor butterfly of each wave of 64 lanes and the serial sum of the waves.  Returns (sum [R], charge [R]):
    charge = sum of |partial sum| over the additions (module docstring)."""
    R, n = t.shape
    per = lanes * width
    sweeps = max(1, -(-n // per))
    tt = torch.nn.functional.pad(t, (0, sweeps * per - n)).view(R, sweeps, lanes, width)
    charge = torch.zeros(R, dtype=t.dtype, device=t.device)
    if presum and width > 1:
        p = tt[..., 0]
        for j in range(1, width):
            p, charge = _add(p, tt[..., j], charge)
        tt = p[..., None]
    acc = torch.zeros(R, lanes, dtype=t.dtype, device=t.device)
    for i in range(sweeps):
        for j in range(tt.shape[-1]):
            acc, charge = _add(acc, tt[:, i, :, j], charge)
    v = acc.view(R, lanes // 64, 64)
    for o in (32, 16, 8, 4, 2, 1):
        v, charge = _add(v[..., :o], v[..., o:2 * o], charge)
    r = v[:, 0, 0]
    for w in range(1, lanes // 64):
        r, charge = _add(r, v[:, w, 0], charge)
    return r, charge


def _rsqrt(t, e_t):
    """rsqrt(t) and its bound given |dt| <= e_t: the graph is convex and decreasing, so the low side is the far one; + RSQRT_ULP ulp."""
    r = torch.rsqrt(t)
    lo = t - e_t
    d = torch.where(lo > 0, torch.rsqrt(lo.clamp_min(1e-300)) - r, torch.full_like(r, float("inf")))
    return r, d + 2 * RSQRT_ULP * U32 * r


# ---------------------------------------------------------------------------------------------------------------------------------------
# norm operand producers
# ---------------------------------------------------------------------------------------------------------------------------------------
def norm_kernel(H, group):
    """launch_norm_rows' choice, all pointers being 16-byte aligned: the 8-wide kernel iff group == 1 and H % 8 == 0."""
    return "rows8" if group == 1 and H % 8 == 0 else "rows4"


def norm_refused(rows, H, group, prec, lo8):
    """Whether launch_norm_rows throws (rows > 0)."""
    return group < 1 or rows % group != 0 or (lo8 and (not prec or group != 1 or H % 128 != 0)) or H % 4 != 0 or H > NORM_MAXC * 256


FORMS = ("single", "split", "lo8")
NORM_CELLS = tuple([("rows8", ln, dt, form, "-") for ln in (True, False) for dt in ("bf16", "f16") for form in FORMS] +
                   [("rows4", ln, dt, form, why) for ln in (True, False) for dt in ("bf16", "f16") for form in ("single", "split")
                    for why in ("H%8==4", "group4")])


def norm_cell(ln, dt, form, H, group):
    k = norm_kernel(H, group)
    return (k, ln, dt, form, "-" if k == "rows8" else "group4" if group == 4 else "H%8==4")


# the GPU file's norm cases: (rows, H, group); every form and type runs on each (the one-byte form where H % 128 == 0 and group == 1)
NORM_ROWS = (1, 3, 5, 257, 513)
NORM_H8 = (8, 128, 512, 520, 640, 3584, 4096)
NORM_H4 = (4, 132, 1028, 4092)
NORM_GROUP4 = tuple((r, h) for h in (64, 1280) for r in (4, 8, 1028))


def norm_shapes():
    """(rows, H, group) of the GPU file: every H at two row counts (rotating through NORM_ROWS so that every row count meets both
    kernels), 257 / 513 rows on the one-byte widths (a second and a third scale tile), and the group-of-4 cases."""
    out = []
    for i, H in enumerate(NORM_H8 + NORM_H4):
        rows = {NORM_ROWS[i % 5], NORM_ROWS[(i + 2) % 5]}
        if H % 128 == 0 and H <= 640:
            rows |= {257, 513}
        if H >= 3584:
            rows = {r if r < 257 else 257 for r in rows}
        out += [(r, H, 1) for r in sorted(rows)]
    out += [(r, H, 4) for r, H in NORM_GROUP4]
    return out


def norm_cases():
    """(rows, H, group, ln, dt, families) of the GPU file: every shape under both norms and both types, all forms of the shape in one
    case, two families per case, rotating so that every family meets every cell."""
    out, n = [], {}
    for rows, H, group in norm_shapes():
        for ln in (True, False):
            for dt in ("bf16", "f16"):
                key = norm_cell(ln, dt, "single", H, group)
                i = n.get(key, 0)
                n[key] = i + 1
                out.append((rows, H, group, ln, dt, (NORM_FAMILIES[i % 6], NORM_FAMILIES[(i + 3) % 6])))
    return out


def norm_forms(H, group):
    return FORMS if group == 1 and H % 128 == 0 else FORMS[:2]


def make_norm(ln, dt, form, rows, H, group, family, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * rows + H + group + (1 if ln else 0))
    x = torch.randn(rows, H, generator=g)
    w = 1 + 0.1 * torch.randn(H, generator=g)
    b = 0.1 * torch.randn(H, generator=g) if ln else None
    eps = 1e-6 if family == "tiny6" else 1e-5
    r = torch.arange(rows)
    if family == "offset":
        x = x + 100
    elif family in ("tiny5", "tiny6"):
        x = x * 1e-3
    elif family == "outlier":
        x[r % 3 == 1] *= 2.0 ** -16                               # values below 2^-14
        x[r[r % 3 == 0], (7 * r[r % 3 == 0]) % H] = 1e4             # one column at 1e4 in an otherwise unit row
        w[H - 1] = 30.0                                           # a gain of 30 on one channel
    elif family == "zero_row":
        x[rows // 2] = 0
    return types.SimpleNamespace(op="norm", ln=ln, dt=dt, form=form, rows=rows, H=H, group=group, family=family, x=x, w=w, b=b, eps=f32(eps),
                                 kernel=norm_kernel(H, group), exact=False)


def _norm_core(x, w, b, eps, width, presum, mutant=None):
    """(y, e): the norm of the rows of x in the kernel's order, in x's dtype, and the bound on the computed y before its output format
    (the producers' (a * rstd) * w and the tail's w * (x * rstd) are the same two roundings)."""
    R, H = x.shape
    ln = b is not None
    per = 64 * width
    sweeps = -(-H // per)
    Hdiv = sweeps * per if mutant == "divides_by_padded_H" else H
    keep = torch.ones(H, dtype=x.dtype, device=x.device)
    if mutant == "sum_misses_last_chunk":
        keep[(sweeps - 1) * per:] = 0
    if ln:
        s, ch = lane_sum(x * keep, 64, width, presum)
        mean = s / Hdiv
        e_mean = U32 * ch / Hdiv + U32 * mean.abs()
        a = x - mean[:, None]
        e_a = e_mean[:, None] + U32 * a.abs()
        sq = a * a
        e_sq = 2 * a.abs() * e_a + e_a * e_a + U32 * sq
    else:
        a, e_a = x, torch.zeros_like(x)
        sq = x * x
        e_sq = U32 * sq
    q, ch = lane_sum(sq * keep, 64, width, presum)
    e_q = (e_sq * keep).sum(dim=1) + U32 * ch
    var = q / Hdiv
    e_var = e_q / Hdiv + U32 * var
    t = var if mutant == "eps_dropped" else var + eps
    rstd, e_r = _rsqrt(t, e_var + U32 * t)
    rstd, e_r = rstd[:, None], e_r[:, None]
    ww = torch.roll(w, 4) if mutant == "weight_shift4" else w
    if mutant == "mean_kept_in_output":
        a = x
    p1 = a * rstd
    e1 = rstd.abs() * e_a + a.abs() * e_r + e_a * e_r + U32 * p1.abs()
    y = ww * p1
    e = ww.abs() * e1 + U32 * y.abs()
    if ln and mutant != "bias_dropped":
        y = y + b
        e = e + U32 * y.abs()
    return y, e


def _group(y, group, transposed=False):
    R, H = y.shape
    if transposed:
        return y.view(group, R // group, H).permute(1, 0, 2).reshape(R // group, group * H)
    return y.reshape(R // group, group * H)


def norm_values(P, dtype, mutant=None):
    """(y, e) [rows / group, H * group] in dtype: the norm's values before the output format."""
    c = lambda t: None if t is None else t.to(dtype)
    width, presum = (8, False) if P.kernel == "rows8" else (4, True)
    y, e = _norm_core(c(P.x), c(P.w), c(P.b), P.eps, width, presum, mutant)
    tr = mutant == "group_rows_transposed"
    return _group(y, P.group, tr), _group(e, P.group, tr)


def norm_encode(y32, dt, form, mutant=None):
    """The output tensors of a norm from its fp32 values y32 (torch float32 or exact fp64): hi (operand type), then nothing / lo
    (operand type) / (e4m3 bytes as fp64 values, E per (row, block))."""
    tdt = TDT[dt]
    y = y32.double()
    hi = round_op(y, dt)
    if form == "single":
        return (hi,)
    r = y - hi
    if mutant == "lo_of_unrounded_hi":                          # the residual taken against y cut (not rounded) to the operand type
        m, ex = torch.frexp(y)
        bits = 8 if dt == "bf16" else 11
        r = y - torch.ldexp(torch.trunc(torch.ldexp(m, torch.full_like(ex, bits))), ex - bits)
    if form == "split":
        return (hi, torch.zeros_like(hi) if mutant == "lo_zero" else r.float().to(tdt).double())
    E = block_E(r)
    q = (r * torch.exp2(127.0 - E)).float().to(torch.float8_e4m3fn).double()
    if mutant == "lo_zero":
        q = torch.zeros_like(q)
    return (hi, q, E)


def norm_decode(parts, P=None, mutant=None):
    """The value the consumer reads out of the output tensors."""
    if len(parts) == 1:
        return parts[0]
    if len(parts) == 2:
        return parts[0] + parts[1]
    hi, q, E = parts
    E = E.double()
    if mutant == "scale_off_by_one":
        E = E + 1
    if mutant == "scale_tile_ignored":                          # the consumer (or the producer) drops row >> 8: rows >= 256 meet the scales of tile 0
        E = E[torch.arange(E.shape[0], device=E.device) & 255]
    return hi + q * torch.exp2(E - 127)


def norm_reference(P, mutant=None, values=None):
    """(y, e_pre, E): the fp64 value the output must decode to, the bound before the output format, the whole bound.  values: the
    result of norm_values(P, float64), which does not depend on the form, when the caller already has it."""
    y, e = values if values is not None else norm_values(P, F64, mutant)
    f16 = P.dt == "f16"
    u = U[P.dt]
    z = y
    if mutant in ("lo_zero", "lo_of_unrounded_hi", "scale_off_by_one", "scale_tile_ignored"):
        y = norm_decode(norm_encode(y, P.dt, P.form, mutant), P, mutant)
    elif f16 and P.form != "lo8":
        lim = 2 * F16_MAX if P.form == "split" else F16_MAX
        y = y.clamp(-lim, lim)
    if P.form == "single":
        E = e + u * y.abs() + (F16_SUB if f16 else 0.0)
    elif P.form == "split":
        E = e + u * (u * y.abs() + (z.abs() - F16_MAX).clamp_min(0) * (1.0 if f16 else 0.0)) + (F16_SUB if f16 else 0.0)
    else:
        ra = u * (z.abs() + e) + ((z.abs() + e - F16_MAX).clamp_min(0) + F16_SUB if f16 else 0.0)
        bmax = ra.view(ra.shape[0], -1, 128).amax(dim=2, keepdim=True).expand(ra.shape[0], ra.shape[1] // 128, 128).reshape(ra.shape)
        E = e + torch.maximum(2.0 ** -4 * ra, 2.0 ** -17 * bmax)
    return y, e, E


def norm_emulate(P):
    y32, _ = norm_values(P, F32)
    return norm_decode(norm_encode(y32, P.dt, P.form))


def norm_naive(P):
    x = P.x.double()
    if P.ln:
        y = torch.nn.functional.layer_norm(x, (P.H,), P.w.double(), P.b.double(), P.eps)
    else:
        y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + P.eps) * P.w.double()
    return y.reshape(P.rows // P.group, P.group * P.H)


def norm_applicable(mutant, P):
    return {
        "mean_kept_in_output": P.ln, "bias_dropped": P.ln, "weight_shift4": P.H > 4,
        "sum_misses_last_chunk": True, "divides_by_padded_H": P.H % (64 * (8 if P.kernel == "rows8" else 4)) != 0,
        "lo_zero": P.form != "single", "lo_of_unrounded_hi": P.form != "single",
        "group_rows_transposed": P.group > 1 and P.rows > P.group,
        "scale_off_by_one": P.form == "lo8", "scale_tile_ignored": P.form == "lo8" and P.rows > 256,
    }.get(mutant, True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# gemm_f32.hip
# ---------------------------------------------------------------------------------------------------------------------------------------
GEMM_M = (1, 31, 33, 127, 129, 257)
GEMM_N = (1, 31, 33, 127, 129, 257)
GEMM_K = (0, 1, 2, 15, 16, 17, 33, 300)
GEMM_ALPHA = (1.0, 2.0 ** -5, 1 / math.sqrt(96))


def pairwise(lists):
    """A small covering design: rows over `lists` such that every pair of values of every two lists occurs in some row (greedy: the
    first three lists by a Latin arrangement, the others chosen row by row for the most new pairs, then rows for what is left)."""
    n = len(lists)
    need = {(i, a, j, b) for i in range(n) for j in range(i + 1, n) for a in range(len(lists[i])) for b in range(len(lists[j]))}
    pairs = lambda row: {(i, row[i], j, row[j]) for i in range(n) for j in range(i + 1, n)}
    rows = []
    l0, l1, l2 = len(lists[0]), len(lists[1]), len(lists[2])
    rest = [range(len(l)) for l in lists[3:]]
    for t in range(max(l0 * l2, l1 * l2, l0 * l1)):
        head = (t % l0, (t % l0 + t // l0) % l1, (t // l0) % l2)
        best = max(itertools.product(*rest), key=lambda r: len(pairs(head + r) & need))
        rows.append(head + best)
        need -= pairs(rows[-1])
    while need:
        i, a, j, b = min(need)
        cands = [r for r in itertools.product(*[range(len(l)) for l in lists]) if r[i] == a and r[j] == b]
        best = max(cands, key=lambda r: len(pairs(r) & need))
        rows.append(best)
        need -= pairs(best)
    return [tuple(l[k] for l, k in zip(lists, r)) for r in rows]


_GEMM_CASES = None


def gemm_cases():
    """(M, N, K, b_nt, b_is_bf16, padded, alpha, family) of the GPU file: pairwise over the issue's lists; every third case `exact`."""
    global _GEMM_CASES
    if _GEMM_CASES is None:
        rows = pairwise([GEMM_M, GEMM_N, GEMM_K, (1, 0), (0, 1), (0, 1), GEMM_ALPHA])
        _GEMM_CASES = [r + (("exact" if r[6] != GEMM_ALPHA[2] and i % 2 == 0 else "normal" if i % 3 else "outlier"),) for i, r in enumerate(rows)]
    return _GEMM_CASES


def make_gemm(M, N, K, b_nt, bf16, padded, alpha, family, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + M * 31 + N * 17 + K)
    if family == "exact":
        A = torch.randint(-8, 9, (M, K), generator=g).float() * 0.25
        B = torch.randint(-4, 5, (N, K), generator=g).float() * 0.5
    else:
        A = torch.randn(M, K, generator=g)
        B = torch.randn(N, K, generator=g) * 0.5
        if family == "outlier" and K:
            A[:, K // 2] *= 300.0
            B[N // 2] *= 1e-3
    if bf16:
        B = B.bfloat16().float()
    Bmem = B if b_nt else B.t().contiguous()                      # as stored: [N, K] or [K, N]
    pa, pb, pc = (3, 5, 7) if padded else (0, 0, 0)
    return types.SimpleNamespace(op="gemm_f32", M=M, N=N, K=K, b_nt=b_nt, bf16=bf16, alpha=f32(alpha), family=family, A=A, Bmem=Bmem,
                                 lda=max(K + pa, 1), ldb=max(Bmem.shape[1] + pb, 1), ldc=N + pc, exact=family == "exact")


def _gemm_operands(P, dtype, mutant):
    A, Bm = P.A.to(dtype), P.Bmem.to(dtype)
    M, N, K = P.M, P.N, P.K
    if mutant == "ld_ignored":                                  # rows addressed with ld = the logical width inside the padded allocations
        buf = torch.full((M, P.lda), POISON, dtype=dtype)
        buf[:, :K] = A
        A = buf.flatten()[:M * K].view(M, K)
    if mutant == "b_transposed":
        Bm = Bm.reshape(Bm.shape[1], Bm.shape[0]).t().contiguous() if Bm.numel() else Bm
    B = Bm if P.b_nt else Bm.t()                                  # [N, K]
    if mutant == "drop_last_ktile" and K:
        B = B.clone()
        B[:, (K - 1) // 16 * 16:] = 0
    if mutant == "odd_k_lost" and K % 2:
        B = B.clone()
        B[:, K - 1] = 0
    if mutant == "row_clamp_leak":
        A = A.clone()
        A[(M - 1) // 128 * 128:] = A[M - 1]
    if mutant == "col_clamp_leak":
        B = B.clone()
        B[(N - 1) // 128 * 128:] = B[N - 1]
    return A, B


def gemm_run(P, dtype, mutant=None):
    """(C, E): alpha * A op(B) as one chain per element in k order, and the bound."""
    A, B = _gemm_operands(P, dtype, mutant)
    acc = torch.zeros(P.M, P.N, dtype=dtype)
    E = torch.zeros(P.M, P.N, dtype=dtype)
    for k0 in range(0, P.K, 2):
        pa = torch.zeros_like(acc)
        for k in range(k0, min(k0 + 2, P.K)):
            p = A[:, k, None] * B[None, :, k]
            acc = acc + p
            pa = pa + p.abs()
        E = E + 2 * U32 * (acc.abs() + pa)
    alpha = 1.0 if mutant == "alpha_dropped" else P.alpha
    y = alpha * acc
    return y, abs(alpha) * E + U32 * y.abs()


def gemm_naive(P):
    B = P.Bmem.double() if P.b_nt else P.Bmem.double().t()
    return P.alpha * (P.A.double() @ B.t())


def gemm_applicable(mutant, P):
    return {
        "drop_last_ktile": P.K > 0, "odd_k_lost": P.K % 2 == 1, "b_transposed": P.N > 1 and P.K > 1, "alpha_dropped": P.alpha != 1.0 and P.K > 0,
        "ld_ignored": P.lda > P.K and P.M > 1 and P.K > 0, "row_clamp_leak": P.M % 128 not in (0, 1) and P.K > 0,
        "col_clamp_leak": P.N % 128 not in (0, 1) and P.K > 0,
    }[mutant]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the fp32 reward tail
# ---------------------------------------------------------------------------------------------------------------------------------------
TAIL_B = (1, 3, 5)
TAIL_D = (64, 100, 260, 3072)
TAIL_VMAX = (1, 5, 255, 256, 257, 1000)


def vb_rows(B, Vmax, k=0):
    """Image-token counts of the B rows: 0, Vmax and all four vb % 4 over the rows of the cases (k rotates the start)."""
    pool = [Vmax, 0] + [v for v in (Vmax - 1, Vmax - 2, Vmax - 3, Vmax // 2, 1, 2, 3) if 0 < v < Vmax]
    return [pool[(k + i) % len(pool)] for i in range(B)]


def _fam_rows(shape, family, g, scale=1.0):
    x = torch.randn(*shape, generator=g) * scale
    if family in ("tiny5", "tiny6"):
        x = x * 1e-3
    elif family == "outlier":
        x[..., shape[-1] // 3] *= 1e3
        x[..., 0] *= 2.0 ** -16
    elif family == "zero_row":
        x[shape[0] // 2] = 0
    elif family == "exact":
        x = torch.randint(-8, 9, shape, generator=g).float() * 0.25
    return x


def make_tail(op, family, seed=0, **kw):
    """Problem of one tail kernel.  Shapes in kw: B, D, Vmax, vb (list), vs (voff_stride), S, use_last_pos, weight, d, attn_o, rows, N, ld,
    has_o, has_u, pad ('left' / 'right')."""
    g = torch.Generator().manual_seed(seed * 104729 + sum(ord(c) for c in op) + sum(int(v) for v in kw.values() if isinstance(v, (int, bool))))
    P = types.SimpleNamespace(op=op, family=family, exact=family == "exact", **kw)
    eps = f32(1e-6 if family == "tiny6" else 1e-5)
    if op in ("ca_scores", "ca_context"):
        B, D, Vmax = P.B, P.D, P.Vmax
        P.vb = [P.vb[0]] * B if P.vs == 0 else list(P.vb)
        counts = P.vb[:1] if P.vs == 0 else P.vb
        P.voff = torch.tensor([0] + list(itertools.accumulate(counts)), dtype=torch.int32)
        if P.vs == 0:                                             # entries a kernel that ignored voff_stride would read: no rows for b >= 1
            P.voff = torch.cat([P.voff, P.voff[-1:].repeat(B - 1)])
        P.ev = _fam_rows((max(int(P.voff[-1]), 1), D), family, g, 0.5)[: int(P.voff[-1])]
        if op == "ca_scores":
            P.kq = _fam_rows((B, D), family, g)
            P.scale = f32(2.0 ** -3 if family == "exact" else 1 / math.sqrt(D))
        else:
            P.pr = torch.rand(B, Vmax, generator=g) / max(Vmax, 1) * 2
            if family == "exact":
                P.pr = torch.randint(0, 9, (B, Vmax), generator=g).float() / 64
    elif op == "gather_norm":
        P.x = _fam_rows((P.B * P.S, P.D), family, g).view(P.B, P.S, P.D)
        last = torch.tensor([(P.S - 1 - 2 * b) % P.S for b in range(P.B)])
        first = torch.tensor([min(b, int(last[b])) // 2 for b in range(P.B)])
        P.tstat = torch.stack([last, first, torch.zeros_like(last), last - first + 1], dim=1).int()
        P.w = 1 + 0.1 * torch.randn(P.D, generator=g) if P.weight else None
        P.eps = eps
    elif op == "rms_rows_f32":
        P.x = _fam_rows((P.rows, P.D), family, g)
        P.w = 1 + 0.1 * torch.randn(P.D, generator=g)
        P.eps = eps
    elif op == "rowvec_linear":
        P.x = _fam_rows((P.B, P.D), family, g)
        P.W = _fam_rows((P.N, P.D), family, g, 0.05 if family != "exact" else 1.0)
    elif op in ("ca_softmax", "ca_softmax_pad"):
        rows, n = (P.B, P.Vmax) if op == "ca_softmax" else (P.rows, P.vb)
        sc = torch.randn(rows, n, generator=g) * 3
        if family == "ramp_hi":
            sc = torch.linspace(90, -20, max(n, 1))[None, :n] + torch.randn(rows, n, generator=g)
        elif family == "all_low":
            sc = -100 - 50 * torch.rand(rows, n, generator=g)
        P.sc = sc
    elif op == "reward_head":
        P.hL = _fam_rows((P.B, P.D), family, g)
        P.o = _fam_rows((P.B, P.D), family, g, 0.5) if P.attn_o else None
        P.ca_w = 1 + 0.1 * torch.randn(P.D, generator=g)
        P.vh = torch.randn(P.d, P.D, generator=g) * 0.05
        P.eps = eps
    elif op == "ca_pool":
        B, S, D = P.B, P.S, P.D
        P.h = _fam_rows((B * S, D), family, g).view(B, S, D)
        P.o = _fam_rows((B * S, D), family, g, 0.5).view(B, S, D) if P.has_o else None
        P.u = _fam_rows((B, D), family, g, 0.5) if P.has_u else None
        P.ca_w = 1 + 0.1 * torch.randn(D, generator=g)
        nvalid = [S, 0, max(S // 2, 1), 1, max(S - 1, 1)][:B] if B > 1 else [S if S == 1 else max(S - 3, 1)]
        m = torch.zeros(B, S, dtype=torch.int64)
        for b, nv in enumerate(nvalid):
            if nv:
                if P.pad == "left":
                    m[b, S - nv:] = 1
                else:
                    m[b, :nv] = 1
        P.mask = m
        P.eps = eps
    else:
        raise ValueError(op)
    return P


def _rms_tail(x, w, eps, mutant=None):
    return _norm_core(x, w, None, eps, 1, False, mutant)


def tail_run(P, dtype, mutant=None):
    """(y, E) of one tail kernel in its own order, in dtype; E the bound (meaningful for float64)."""
    c = lambda t: None if t is None else t.to(dtype)
    op = P.op
    if op == "rms_rows_f32":
        return _rms_tail(c(P.x), c(P.w), P.eps, mutant)
    if op == "gather_norm":
        idx = torch.full((P.B,), P.S - 1, dtype=torch.long) if P.use_last_pos else P.tstat[:, 0].long()
        if mutant == "gathers_first_valid":
            idx = P.tstat[:, 1].long()
        if mutant == "last_valid_off_by_one":
            idx = torch.where(idx > 0, idx - 1, idx + 1).clamp_max(P.S - 1)
        xr = c(P.x)[torch.arange(P.B), idx]
        if P.w is None:
            return xr, torch.zeros_like(xr)
        return _rms_tail(xr, c(P.w), P.eps, mutant)
    if op == "rowvec_linear":
        x, W = c(P.x), c(P.W)
        if mutant == "head_k_reads_row0":
            W = W[:1].expand_as(W)
        t = x[:, None, :] * W[None, :, :]                          # [B, N, K]
        if mutant == "sum_misses_last_chunk":
            t = t.clone()
            t[..., (-(-P.D // 256) - 1) * 256:] = 0
        s, ch = lane_sum(t.reshape(-1, P.D), 64, 4, True)
        E = U32 * (t.abs().reshape(-1, P.D).sum(dim=1) + ch)
        return s.view(P.B, P.N), E.view(P.B, P.N)
    if op == "ca_scores":
        B, D, Vmax = P.B, P.D, P.Vmax
        ev, kq = c(P.ev), c(P.kq)
        vs = P.vs if mutant != "voff_stride_ignored" else 1 - P.vs
        sc = torch.zeros(B, Vmax, dtype=dtype)
        E = torch.zeros(B, Vmax, dtype=dtype)
        scale = 1.0 if mutant == "scale_dropped" else P.scale
        nrows = ev.shape[0]
        for b in range(B):
            i0 = min(b * vs, len(P.voff) - 2)
            v0, vb = int(P.voff[i0]), int(P.voff[i0 + 1] - P.voff[i0])
            n = min(Vmax, nrows - v0) if mutant == "pad_scores_read_next_row" else min(vb, Vmax)
            if n <= 0:
                continue
            t = ev[v0:v0 + n] * kq[b][None, :]
            if mutant == "sum_misses_last_chunk":
                t = t.clone()
                t[:, (-(-D // 256) - 1) * 256:] = 0
            s, ch = lane_sum(t, 64, 4, True)
            sc[b, :n] = s * scale
            E[b, :n] = abs(scale) * U32 * (t.abs().sum(dim=1) + ch) + U32 * sc[b, :n].abs()
        return sc, E
    if op in ("ca_softmax", "ca_softmax_pad"):
        r = c(P.sc)
        rows, n = r.shape
        npad = 0 if op == "ca_softmax" else P.Vmax - P.vb
        if mutant == "pad_term_dropped":
            npad = 0
        if n == 0:
            return r, torch.zeros_like(r)
        mx = r.max(dim=1).values
        if npad > 0:
            mx = mx.clamp_min(0)
        if mutant == "no_max_subtraction":
            mx = torch.zeros_like(mx)
        arg = r - mx[:, None]
        e = torch.exp(arg)
        if mutant == "no_max_subtraction":
            e = e.float().to(dtype)                               # what overflows in fp32 overflows
        e_e = e * (U32 * arg.abs() + 2 * U32) + F32_MIN
        s, ch = lane_sum(e, 256, 1, False)
        e_s = e_e.sum(dim=1) + U32 * ch
        if npad > 0:
            pe = torch.exp(-mx)
            pt = npad * pe
            s2 = s + pt
            e_s = e_s + npad * pe * 2 * U32 + U32 * pt + U32 * s2
            s = s2
        inv = 1 / s
        e_inv = e_s / (s * (s - e_s).clamp_min(1e-300)) + U32 * inv
        y = e * inv[:, None]
        E = inv[:, None] * e_e + e * e_inv[:, None] + e_e * e_inv[:, None] + U32 * y + F32_MIN
        return y, E
    if op == "ca_context":
        B, D, Vmax = P.B, P.D, P.Vmax
        ev, pr = c(P.ev), c(P.pr)
        vs = P.vs if mutant != "voff_stride_ignored" else 1 - P.vs
        ctx = torch.zeros(B, D, dtype=dtype)
        E = torch.zeros(B, D, dtype=dtype)
        for b in range(B):
            i0 = min(b * vs, len(P.voff) - 2)
            v0, vb = int(P.voff[i0]), int(P.voff[i0 + 1] - P.voff[i0])
            t = pr[b, :vb, None] * ev[v0:v0 + vb]                  # [vb, D]
            v4 = vb // 4 * 4
            a = torch.zeros(4, D, dtype=dtype)
            chE = torch.zeros(4, D, dtype=dtype)
            for j in range(0, v4, 4):
                a = a + t[j:j + 4]
                chE = chE + a.abs()
            a0, c0 = a[0], chE[0]
            if mutant != "context_tail_dropped":
                for j in range(v4, vb):
                    a0 = a0 + t[j]
                    c0 = c0 + a0.abs()
            s01, s23 = a0 + a[1], a[2] + a[3]
            y = s01 + s23
            ctx[b] = y
            E[b] = U32 * (t.abs().sum(dim=0) + c0 + chE[1] + chE[2] + chE[3] + s01.abs() + s23.abs() + y.abs())
        return ctx, E
    if op == "reward_head":
        h, vh = c(P.hL), c(P.vh)
        if mutant == "head_k_reads_row0":
            vh = vh[:1].expand_as(vh)
        if P.o is None:
            v, e_v = h, torch.zeros_like(h)
        else:
            v0 = h + c(P.o)
            e0 = U32 * v0.abs()
            sq = v0 * v0
            s, ch = lane_sum(sq, 256, 1, False)
            e_s = (2 * v0.abs() * e0 + e0 * e0 + U32 * sq).sum(dim=1) + U32 * ch
            var = s / P.D
            t = var + P.eps
            rstd, e_r = _rsqrt(t, e_s / P.D + U32 * var + U32 * t)
            rstd, e_r = rstd[:, None], e_r[:, None]
            if mutant == "no_ca_norm":
                rstd, e_r = torch.ones_like(rstd), torch.zeros_like(e_r)
            p1 = v0 * rstd
            e1 = rstd * e0 + v0.abs() * e_r + e0 * e_r + U32 * p1.abs()
            w = c(P.ca_w)
            v = w * p1
            e_v = w.abs() * e1 + U32 * v.abs()
        t = v[:, None, :] * vh[None, :, :]                         # [B, d, D]
        e_t = vh.abs()[None] * e_v[:, None, :] + U32 * t.abs()
        s, ch = lane_sum(t.reshape(-1, P.D), 256, 1, False)
        E = e_t.reshape(-1, P.D).sum(dim=1) + U32 * ch
        return s.view(P.B, P.d), E.view(P.B, P.d)
    if op == "ca_pool":
        B, S, D = P.B, P.S, P.D
        h = c(P.h)
        ca = P.o is not None or P.u is not None
        w = c(P.ca_w) if ca else None
        out = torch.zeros(B, D, dtype=dtype)
        E = torch.zeros(B, D, dtype=dtype)
        for b in range(B):
            valid = torch.nonzero(P.mask[b]).flatten() if mutant != "pool_counts_pads" else torch.arange(S)
            cnt = float(S) if mutant == "pool_divides_by_S" else float(len(valid))
            acc = torch.zeros(D, dtype=dtype)
            e_acc = torch.zeros(D, dtype=dtype)
            if len(valid):
                v = h[b, valid]
                e_v = torch.zeros_like(v)
                if P.u is not None and mutant != "pool_u_after_norm":
                    v = v + c(P.u)[b]
                    e_v = U32 * v.abs()
                if P.o is not None:
                    v = v + c(P.o)[b, valid]
                    e_v = e_v + U32 * v.abs()
                if ca:
                    sq = v * v
                    s, ch = lane_sum(sq, 256, 1, False)
                    e_s = (2 * v.abs() * e_v + e_v * e_v + U32 * sq).sum(dim=1) + U32 * ch
                    var = s / D
                    t = var + P.eps
                    rstd, e_r = _rsqrt(t, e_s / D + U32 * var + U32 * t)
                    rstd, e_r = rstd[:, None], e_r[:, None]
                    p1 = v * rstd
                    e1 = rstd * e_v + v.abs() * e_r + e_v * e_r + U32 * p1.abs()
                    v = w * p1
                    e_v = w.abs() * e1 + U32 * v.abs()
                    if mutant == "pool_u_after_norm" and P.u is not None:
                        v = v + c(P.u)[b]
                for i in range(v.shape[0]):
                    acc = acc + v[i]
                    e_acc = e_acc + e_v[i] + (U32 * acc.abs() if i else 0.0)
            inv = 1 / max(cnt, 1e-8)
            inv = torch.tensor(inv, dtype=dtype).item()
            y = acc * inv
            out[b] = y
            E[b] = inv * e_acc + 2 * U32 * y.abs()
        return out, E
    raise ValueError(op)


def tail_naive(P):
    """The same operation written at once in torch fp64."""
    d = lambda t: t.double()
    op = P.op
    rms = lambda x, w, eps: w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))
    if op == "rms_rows_f32":
        return rms(d(P.x), d(P.w), P.eps)
    if op == "gather_norm":
        xr = d(P.x)[torch.arange(P.B), (torch.full((P.B,), P.S - 1) if P.use_last_pos else P.tstat[:, 0].long())]
        return xr if P.w is None else rms(xr, d(P.w), P.eps)
    if op == "rowvec_linear":
        return d(P.x) @ d(P.W).t()
    if op in ("ca_scores", "ca_context"):
        out = torch.zeros(P.B, P.Vmax if op == "ca_scores" else P.D, dtype=F64)
        for b in range(P.B):
            v0, v1 = int(P.voff[b * P.vs]), int(P.voff[b * P.vs + 1])
            if op == "ca_scores":
                out[b, :v1 - v0] = P.scale * (d(P.ev)[v0:v1] @ d(P.kq)[b])
            else:
                out[b] = d(P.pr)[b, :v1 - v0] @ d(P.ev)[v0:v1]
        return out
    if op == "ca_softmax":
        return torch.softmax(d(P.sc), dim=1)
    if op == "ca_softmax_pad":
        full = torch.cat([d(P.sc), torch.zeros(P.rows, P.Vmax - P.vb, dtype=F64)], dim=1)
        return torch.softmax(full, dim=1)[:, :P.vb]
    if op == "reward_head":
        v = d(P.hL) if P.o is None else rms(d(P.hL) + d(P.o), d(P.ca_w), P.eps)
        return v @ d(P.vh).t()
    if op == "ca_pool":
        v = d(P.h)
        if P.o is not None or P.u is not None:
            v = rms(v + (d(P.o) if P.o is not None else 0) + (d(P.u)[:, None, :] if P.u is not None else 0), d(P.ca_w), P.eps)
        m = d(P.mask)
        return (v * m[:, :, None]).sum(dim=1) / m.sum(dim=1).clamp_min(1e-8)[:, None]
    raise ValueError(op)


def tail_applicable(mutant, P):
    op = P.op
    if op == "gather_norm":
        return {"gathers_first_valid": not P.use_last_pos and P.S > 1, "last_valid_off_by_one": P.S > 1,
                "eps_dropped": P.w is not None, "weight_shift4": P.w is not None}[mutant]
    if op == "rowvec_linear":
        return {"head_k_reads_row0": P.N > 1}.get(mutant, True)
    if op == "ca_scores":
        tot = int(P.voff[-1])
        return {"pad_scores_read_next_row": P.vs == 1 and any(P.vb[b] < P.Vmax and tot - int(P.voff[b]) > P.vb[b] for b in range(P.B)),
                "voff_stride_ignored": P.B > 1 and any(v > 0 for v in P.vb)}.get(mutant, True)
    if op == "ca_context":
        return {"context_tail_dropped": any(v % 4 for v in P.vb), "voff_stride_ignored": P.B > 1 and any(v > 0 for v in P.vb)}[mutant]
    if op == "ca_softmax_pad":
        return {"pad_term_dropped": P.Vmax > P.vb}.get(mutant, True)
    if op == "reward_head":
        return {"no_ca_norm": P.o is not None, "head_k_reads_row0": P.d > 1}[mutant]
    if op == "ca_pool":
        return {"pool_counts_pads": bool((P.mask == 0).any()), "pool_divides_by_S": bool(((P.mask.sum(dim=1) != P.S) & (P.mask.sum(dim=1) > 0)).any()),
                "pool_u_after_norm": P.u is not None}[mutant]
    return True


# the GPU file's tail cases: op -> list of kwargs of make_tail
def tail_cases():
    cs = {k: [] for k in TAIL_MUTANTS}
    for i, Vmax in enumerate(TAIL_VMAX):
        B, D = TAIL_B[i % 3], TAIL_D[i % 4]
        for vs in (1, 0):
            if Vmax == 1000 and D == 3072:
                D = 260
            vb = vb_rows(B, Vmax, i)
            if vs == 0:
                vb = [max(Vmax - (i % 4), 0 if Vmax > 1 else 1)] * B
            cs["ca_scores"].append(dict(B=B, D=D, Vmax=Vmax, vb=vb, vs=vs))
            cs["ca_context"].append(dict(B=B, D=D, Vmax=Vmax, vb=vb, vs=vs))
        cs["ca_softmax"].append(dict(B=B, Vmax=Vmax))
    cs["ca_scores"].append(dict(B=3, D=3072, Vmax=5, vb=[5, 0, 3], vs=1))
    cs["ca_context"].append(dict(B=5, D=3072, Vmax=257, vb=[257, 0, 254, 255, 129], vs=1))
    for Vmax, vb, extra in [(1, 1, 0), (5, 2, 3), (255, 255, 1), (256, 1, 0), (257, 256, 4), (257, 257, 0), (1000, 997, 8), (1000, 1000, 0)]:
        cs["ca_softmax_pad"].append(dict(rows=3 if Vmax != 257 else 5, vb=vb, Vmax=Vmax, ld=(vb + extra + 3) // 4 * 4))
    for i, D in enumerate(TAIL_D):
        B = TAIL_B[i % 3]
        for ulp in (0, 1):
            for weight in (True, False):
                cs["gather_norm"].append(dict(B=B, S=7 if i % 2 else 1 + i, D=D, use_last_pos=ulp, weight=weight))
        cs["rms_rows_f32"].append(dict(rows=(1, 3, 5, 9)[i], D=D))
        cs["rowvec_linear"].append(dict(B=B, N=(1, 5, 66, 7)[i], D=D))
        for d in (1, 2, 10):
            for attn_o in (True, False):
                if (i + d) % 2 == 0 or D == 100:
                    cs["reward_head"].append(dict(B=TAIL_B[(i + d) % 3], D=D, d=d, attn_o=attn_o))
    k = 0
    for D, S, B in [(64, 300, 5), (100, 1, 1), (260, 300, 3), (3072, 5, 5), (4096, 7, 3), (4096, 1, 5)]:
        for has_o, has_u in [(True, True), (True, False), (False, True), (False, False)]:
            if D in (64, 4096) or (k % 4) == (2 * has_o + has_u):
                cs["ca_pool"].append(dict(B=B, S=S, D=D, has_o=has_o, has_u=has_u, pad="left" if k % 2 else "right"))
            k += 1
    return cs
