"""The floating-point row kernels on their own (lr_op_norm_rows_ex, lr_op_gemm_f32 and the nine kernels of the fp32 reward tail)
against the fp64 reference and per-element rounding bound of tests/helpers/rowops_ref.py, at the shapes where each kernel changes path.
Inputs sit in allocations whose unused rows and columns hold poison (3e4, or NaN where a leak would otherwise be masked); outputs sit
between sentinel guard rows, with sentinel gap columns and sentinel scale bytes, and every launch checks that nothing else was written.
All pointers are 16-byte aligned and all indices in range; refusals are tested through LR_EINVAL of calls that launch nothing.  On the
`exact` family the output is compared bit for bit.  Every case prints max err / bound; the last test prints the largest per kernel."""
import ctypes as C

import pytest
import torch

from helpers import gemm_ref as gr
from helpers import rowops_ref as rr
from helpers.guards import DEV, GR, S8, Out, P, _in, _stream
from llava_reward_amd import _lib as L

pytestmark = pytest.mark.gpu

CODE = {"bf16": L.LR_DT_BF16, "f16": L.LR_DT_F16}
F64 = torch.float64
NAN = float("nan")
LR_EINVAL = 1                  # include/llava_reward_hip.h
RATIOS = {}                    # kernel and form -> largest err / bound seen (printed by the last test)
CELLS = set()                  # norm cells reached


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return L.load()


def _note(key, worst):
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst)


def _compare(key, label, got, y, E, exact=False):
    err = (got.double().cpu() - y).abs()
    worst = rr.ratio(err, E)
    bits = exact and torch.equal(got.float().cpu(), y.float())
    print(f"[{key} {label}] max err/bound {worst:.3g}  max err {err.max().item() if err.numel() else 0.0:.3g}{'  bits equal' if bits else ''}")
    if exact:
        assert bits, (key, label, "exact family: output bits differ from the fp64 reference")
    if worst > 1.0:
        r = torch.where(E > 0, err / E.clamp_min(1e-300), (err > 0).double() * 1e300)
        i = int(torch.where(torch.isfinite(r), r, torch.full_like(r, 1e300)).argmax())
        print(f"  worst element {i} of shape {tuple(y.shape)}: got {got.flatten()[i].item()!r} want {y.flatten()[i].item()!r} bound {E.flatten()[i].item():.3g}")
    assert worst <= 1.0, (key, label, worst)
    _note(key, worst)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------------
# norm operand producers
# ---------------------------------------------------------------------------------------------------------------------------------------
def _norm_launch(lib, Pn, form, xd, wd, bd):
    """One lr_op_norm_rows_ex launch; returns (Out, scales or None, used scale index or None)."""
    rows, H, g = Pn.rows, Pn.H, Pn.group
    prec = 0 if form == "single" else 1
    out = Out(rows // g, (H * g) << prec, dtype=gr.TDT[Pn.dt])
    scales = idx = None
    if form == "lo8":
        scales = torch.full((lib.lr_op_lo8_scratch_bytes(rows, H) + 256,), S8, dtype=torch.uint8, device=DEV)
        idx = rr.lo8_scale_index(rows, H, DEV)
    rc = lib.lr_op_norm_rows_ex(P(xd), P(wd), P(bd), out.ptr, rows, H, Pn.eps, CODE[Pn.dt], prec, g, P(scales), _stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, form)
    out.check(f"norm {form}")
    return out, scales, idx


@pytest.mark.parametrize("case", rr.norm_cases(), ids=lambda c: f"{c[0]}x{c[1]}g{c[2]}-{'ln' if c[3] else 'rms'}-{c[4]}")
def test_norm_rows_every_form(lib, case):
    rows, H, group, ln, dt, fams = case
    for fam in fams:
        base = rr.make_norm(ln, dt, "single", rows, H, group, fam)
        xd, wd = _in(base.x), _in(base.w, extra_rows=0, ld=H + 8).view(-1)
        bd = _in(base.b, extra_rows=0, ld=H + 8).view(-1) if ln else None
        values = rr.norm_values(base, F64)
        W = H * group
        hi_single = None
        for form in rr.norm_forms(H, group):
            Pn = rr.make_norm(ln, dt, form, rows, H, group, fam)
            assert Pn.kernel == rr.norm_kernel(H, group)
            CELLS.add(rr.norm_cell(ln, dt, form, H, group))
            out, scales, idx = _norm_launch(lib, Pn, form, xd, wd, bd)
            y, e, E = rr.norm_reference(Pn, values=values)
            hi = out.body[:, :W]
            if form == "single":
                hi_single = hi.clone()
                got = hi.double()
            else:
                assert torch.equal(hi.view(torch.int16), hi_single.view(torch.int16)), (form, "the hi half differs from the single-operand output")
                if form == "split":
                    got = hi.double() + out.body[:, W:].double()
                else:
                    raw = out.all[GR:GR + rows, H:2 * H].contiguous().view(torch.uint8)                # 2H bytes: H of e4m3, H untouched
                    assert bool((raw[:, H:] == S8).all()), "write behind the one-byte residual half"
                    used = torch.zeros(scales.numel(), dtype=torch.bool, device=DEV)
                    used[idx.flatten()] = True
                    assert bool((scales[~used] == S8).all()), "write into unused scale bytes"
                    Ed = rr.lo8_scales_decode(scales, rows, H)
                    assert torch.equal(Ed, scales[idx])                                              # the port and the decode agree on the device's bytes
                    q = raw[:, :H].contiguous().view(torch.float8_e4m3fn).double()
                    got = hi.double() + (q.view(rows, H // 128, 128) * torch.exp2(Ed.double() - 127)[:, :, None]).view(rows, H)
                    # every scale byte inside what the reference residuals (against the device's own hi) allow
                    r = (y - hi.double().cpu()).abs().view(rows, H // 128, 128)
                    amax, emax = r.amax(dim=2), e.view(rows, H // 128, 128).amax(dim=2)
                    lo_E, hi_E = rr.e8m0_of_amax((amax - emax).clamp_min(0)), rr.e8m0_of_amax(amax + emax)
                    Ec = Ed.cpu().long()
                    ok = ((Ec >= lo_E) & (Ec <= hi_E)) | ((amax - emax <= 0) & ((Ec == 127) | (Ec <= hi_E)))
                    assert bool(ok.all()), ("scale byte outside the reference interval", int((~ok).sum()))
                    if fam == "zero_row" and not ln:
                        z = rows // 2
                        assert bool((raw[z, :H] == 0).all()) and bool((Ec[z] == 127).all()) and bool((hi[z].view(torch.int16) == 0).all())
            # (hi + lo against fp64 with the device's own hi: the same comparison, the bound's residual term being its output-format part)
            _compare(f"norm_{Pn.kernel}/{form}/{dt}", f"{'ln' if ln else 'rms'} {rows}x{H} g{group} {fam}", got, y, E)
            if fam == "zero_row" and not ln:                    # RMSNorm of an all-zero row is exactly 0 in every form
                z, c0 = divmod(rows // 2, group)
                assert bool((got[z, c0 * H:(c0 + 1) * H] == 0).all())


def test_norm_lo8_output_feeds_the_e4m3_residual_pass(lib):
    """Producer to consumer: the one-byte output of the norm goes into lr_op_gemm_bt_mixed WITHOUT flag 2, the norm's scale array as the
    GEMM's scratch; against fp64 of (hi + dec(lo8)) W^T under gemm_ref's bound for an A that is already encoded (q(A_lo) = 0)."""
    M, K, N, dt = 257, 640, 256, "f16"
    tdt = gr.TDT[dt]
    Pn = rr.make_norm(False, dt, "lo8", M, K, 1, "normal", seed=3)
    out, scales, idx = _norm_launch(lib, Pn, "lo8", _in(Pn.x), _in(Pn.w, extra_rows=0, ld=K + 8).view(-1), None)
    g = torch.Generator().manual_seed(11)
    Wt = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16).to(tdt)
    hi = out.body[:, :K].double().cpu()
    raw = out.all[GR:GR + M, K:2 * K].contiguous().view(torch.uint8)[:, :K].contiguous()
    Ed = rr.lo8_scales_decode(scales, M, K).double().cpu()
    lo = (raw.view(torch.float8_e4m3fn).double().cpu().view(M, K // 128, 128) * torch.exp2(Ed - 127)[:, :, None]).view(M, K)
    Wd = Wt.double()
    qw = gr.qerr(Wd, gr.e8m0_of_amax(Wd.abs().amax()))
    Pg = gr.Problem(kform="e4m3", family="normal", dt=dt, M=M, N=N, K=K, k2=0, epi=gr.EPI_OUT_F32, act=0, exact=False, lo8_out=False,
                    kernel="product", rope_cols=0, rope_hd=0, bias=None, res=None, split_out=False, nout=N, cs=None, ascale=None, wscale=None,
                    qterm=lo.abs() @ qw.T, dropped=None, t8_ops=[(lo.abs(), Wd.abs() + qw)],
                    segs=[("a_hi x w", hi, Wd, 32), ("a_lo x w [e4m3]", lo, Wd, 128)])
    y, E = gr.reference(Pg)
    A = _in(out.body)                                           # [M, 2K] 16-bit words: hi | bytes | untouched; poisoned rows behind
    cout = Out(M, N)
    W8 = torch.zeros(N + GR, K, dtype=tdt, device=DEV)
    wexp = (C.c_int * 2)(0, 0)
    Wdev = _in(Wt)
    rc = lib.lr_op_gemm_bt_mixed(P(A), P(Wdev), P(W8), P(scales), cout.ptr, None, M, N, K, gr.EPI_OUT_F32, 0, CODE[dt], 1, wexp, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    cout.check("consumer")
    assert torch.equal(A[:M].view(torch.int16), out.body.view(torch.int16)), "the consumer changed its A"
    _compare("norm_rows8/lo8->gemm_e4m3", f"M={M} K={K} N={N}", cout.body, y, E)
    full = (Pn.x.double() * torch.rsqrt(Pn.x.double().pow(2).mean(-1, keepdim=True) + Pn.eps) * Pn.w.double()) @ Wd.T
    print(f"  chain against fp64 of the un-rounded norm: {((cout.body.double().cpu() - full).abs().max() / full.abs().max()).item():.2e} of the output scale")


def test_norm_refusals_launch_nothing(lib):
    x = _in(torch.zeros(8, 4100))
    w = _in(torch.ones(4100), extra_rows=0).view(-1)
    out = Out(8, 2 * 4100, dtype=torch.float16)
    scales = torch.full((lib.lr_op_lo8_scratch_bytes(8, 4096) + 256,), S8, dtype=torch.uint8, device=DEV)
    for rows, H, prec, group, lo8 in [(8, 6, 0, 1, False), (8, 4100, 0, 1, False), (5, 64, 0, 4, False), (8, 128, 0, 1, True), (8, 128, 1, 2, True),
                                      (8, 192, 1, 1, True)]:
        assert rr.norm_refused(rows, H, group, prec, lo8)
        rc = lib.lr_op_norm_rows_ex(P(x), P(w), None, out.ptr, rows, H, 1e-5, CODE["f16"], prec, group, P(scales) if lo8 else None, _stream())
        torch.cuda.synchronize()
        assert rc == LR_EINVAL, (rows, H, prec, group, lo8, rc)
        assert out.untouched() and bool((scales == S8).all())


def test_every_norm_cell_was_reached():
    assert CELLS == set(rr.NORM_CELLS), set(rr.NORM_CELLS) - CELLS


# ---------------------------------------------------------------------------------------------------------------------------------------
# gemm_f32.hip
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rr.gemm_cases(), ids=lambda c: "-".join(f"{v:.3g}" if isinstance(v, float) else str(v) for v in c))
def test_gemm_f32(lib, case):
    M, N, K, b_nt, bf16, padded, alpha, fam = case
    Pg = rr.make_gemm(*case)
    A = _in(Pg.A, ld=Pg.lda)
    Bm = Pg.Bmem.bfloat16().view(torch.int16) if bf16 else Pg.Bmem
    Bd = _in(Bm, fill=int(torch.tensor(gr.POISON).bfloat16().view(torch.int16)) if bf16 else gr.POISON, ld=Pg.ldb)
    out = Out(M, N, ld=Pg.ldc)
    rc = lib.lr_op_gemm_f32(P(A), P(Bd), bf16, b_nt, out.ptr, M, N, K, Pg.lda, Pg.ldb, Pg.ldc, Pg.alpha, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    out.check("gemm_f32")
    y, E = rr.gemm_run(Pg, F64)
    if K == 0:
        assert bool((out.body == 0).all()), "K = 0 must write zeros"
    _compare(f"gemm_f32/{'nt' if b_nt else 'nn'}/{'bf16' if bf16 else 'f32'}", f"M={M} N={N} K={K} ld=({Pg.lda},{Pg.ldb},{Pg.ldc}) alpha={alpha:.4g} {fam}",
             out.body, y, E, exact=Pg.exact)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the fp32 reward tail
# ---------------------------------------------------------------------------------------------------------------------------------------
def _run_tail(lib, Pt):
    """One launch of the tail kernel of Pt; returns the output rows (device) after the guard checks."""
    op, st = Pt.op, _stream()
    keep = []                                                   # every device buffer lives until the launch has finished

    def _buf(t, **kw):
        keep.append(_in(t, **kw))
        return keep[-1]

    def _dev(t):
        keep.append(t.to(DEV))
        return keep[-1]

    if op == "rms_rows_f32":
        out = Out(Pt.rows, Pt.D)
        rc = lib.lr_op_rms_rows_f32(P(_buf(Pt.x)), P(_buf(Pt.w, extra_rows=0, ld=Pt.D + 8)), Pt.eps, out.ptr, Pt.rows, Pt.D, st)
    elif op == "gather_norm":
        out = Out(Pt.B, Pt.D)
        w = _buf(Pt.w, extra_rows=0, ld=Pt.D + 8) if Pt.w is not None else None
        assert int(Pt.tstat[:, :2].min()) >= 0 and int(Pt.tstat[:, :2].max()) < Pt.S
        rc = lib.lr_op_gather_norm_rows(P(_buf(Pt.x, fill=NAN)), P(_dev(Pt.tstat)), Pt.S, Pt.use_last_pos, P(w), Pt.eps, out.ptr, Pt.B, Pt.D, st)
    elif op == "rowvec_linear":
        out = Out(Pt.B, Pt.N)
        rc = lib.lr_op_rowvec_linear(P(_buf(Pt.x)), P(_buf(Pt.W)), out.ptr, Pt.B, Pt.N, Pt.D, st)
    elif op == "ca_scores":
        out = Out(Pt.B, Pt.Vmax)
        assert int(Pt.voff.min()) >= 0 and int(Pt.voff.max()) <= Pt.ev.shape[0]
        rc = lib.lr_op_ca_scores(P(_buf(Pt.ev, fill=NAN)), P(_buf(Pt.kq)), P(_dev(Pt.voff)), Pt.B, Pt.Vmax, Pt.D, Pt.scale, out.ptr, Pt.vs, st)
    elif op == "ca_softmax":
        out = Out(Pt.B, Pt.Vmax)
        out.body.copy_(Pt.sc.to(DEV))
        rc = lib.lr_op_ca_softmax(out.ptr, Pt.B, Pt.Vmax, st)
    elif op == "ca_softmax_pad":
        out = Out(Pt.rows, Pt.ld)                                 # columns vb .. ld hold NaN and must stay as they are
        out.body.fill_(NAN)
        out.body[:, :Pt.vb] = Pt.sc.to(DEV)
        before = out.body[:, Pt.vb:].clone().view(torch.int32)
        rc = lib.lr_op_ca_softmax_pad(out.ptr, Pt.rows, Pt.ld, Pt.vb, Pt.Vmax, st)
        torch.cuda.synchronize()
        assert torch.equal(out.body[:, Pt.vb:].view(torch.int32), before), "ca_softmax_pad wrote past vb"
    elif op == "ca_context":
        out = Out(Pt.B, Pt.D)
        pr = Pt.pr.clone()
        for b in range(Pt.B):
            pr[b, Pt.vb[b]:] = NAN                              # probabilities of the padding rows are never read
        rc = lib.lr_op_ca_context(P(_buf(Pt.ev, fill=NAN)), P(_buf(pr, fill=NAN)), P(_dev(Pt.voff)), Pt.B, Pt.Vmax, Pt.D, out.ptr, Pt.vs, st)
    elif op == "reward_head":
        out = Out(Pt.B, Pt.d)
        o = _buf(Pt.o) if Pt.o is not None else None
        rc = lib.lr_op_reward_head(P(_buf(Pt.hL)), P(o), P(_buf(Pt.ca_w, extra_rows=0, ld=Pt.D + 8)), Pt.eps, P(_buf(Pt.vh)), Pt.d, out.ptr, Pt.B, Pt.D, st)
    elif op == "ca_pool":
        out = Out(Pt.B, Pt.D)
        o = _buf(Pt.o) if Pt.o is not None else None
        u = _buf(Pt.u) if Pt.u is not None else None
        rc = lib.lr_op_ca_pool(P(_buf(Pt.h)), P(o), P(u), P(_buf(Pt.ca_w, extra_rows=0, ld=Pt.D + 8)), Pt.eps, P(_dev(Pt.mask)), out.ptr, Pt.B, Pt.S, Pt.D, st)
    else:
        raise ValueError(op)
    torch.cuda.synchronize()
    assert rc == 0, (op, rc)
    out.check(op)
    return out


TAIL_CASES = [(op, kw) for op, cases in rr.tail_cases().items() for kw in cases]


@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: c[0] + "-" + "-".join(f"{k}{v if not isinstance(v, list) else '_'.join(map(str, v))}" for k, v in c[1].items()))
def test_reward_tail(lib, case):
    op, kw = case
    for fam in rr.TAIL_FAMILIES[op]:
        if fam == "all_low" and kw["Vmax"] == kw["vb"]:
            continue
        Pt = rr.make_tail(op, fam, **kw)
        y, E = rr.tail_run(Pt, F64)
        out = _run_tail(lib, Pt)
        cols = {"ca_softmax_pad": Pt.vb if op == "ca_softmax_pad" else 0}.get(op) or out.cols
        got = out.body[:, :cols]
        copy = op == "gather_norm" and Pt.w is None
        _compare(op, f"{kw} {fam}", got, y, E, exact=Pt.exact or copy)
        if op == "ca_scores":
            for b in range(Pt.B):
                assert bool((got[b, Pt.vb[b]:].view(torch.int32) == 0).all()), "a padded score is not exactly 0.0"
        if op == "ca_pool":
            empty = (Pt.mask.sum(dim=1) == 0).to(DEV)
            assert bool((got[empty] == 0).all()), "an all-padding row does not pool to exactly 0"


def test_tail_refusals_launch_nothing(lib):
    st = _stream()
    x = _in(torch.zeros(2, 4100))
    out = Out(2, 4100)
    voff = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)
    mask = torch.ones(2, 1, dtype=torch.int64, device=DEV)
    assert lib.lr_op_rowvec_linear(P(x), P(x), out.ptr, 2, 2, 6, st) == LR_EINVAL
    assert lib.lr_op_ca_scores(P(x), P(x), P(voff), 2, 1, 6, 1.0, out.ptr, 1, st) == LR_EINVAL
    assert lib.lr_op_ca_pool(P(x), None, None, None, 1e-5, P(mask), out.ptr, 2, 1, 4100, st) == LR_EINVAL
    torch.cuda.synchronize()
    assert out.untouched()


def test_zz_report_largest_ratio_per_kernel():
    print("\nlargest max err / bound per kernel and form:")
    for k in sorted(RATIOS):
        print(f"  {k:40s} {RATIOS[k]:.3g}")
    assert RATIOS and all(v <= 1.0 for v in RATIOS.values())
