"""CPU checks of tests/helpers/gemm_ref.py, the fp64 reference and per-element bound the GEMM kernel tests assert against: the
reference is the plain fp64 operation, the `exact` family is exact, the bound has the scale of its rounding model, every mutant of the
reference is caught at every (K-loop form, K) the GPU file uses, and the dispatch table covers every instantiation the sources can
launch and nothing else."""
import os

import pytest
import torch

from helpers import gemm_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "llava-reward_amd", "csrc")

# (epi, act, bias, one-byte residual output) per K-loop form, for the reference and mutant checks
EPIS = [(gr.EPI_OUT_F32, 0, True, False), (gr.EPI_RESADD_F32, 0, False, False), (gr.EPI_OUT_OP, 0, True, False),
        (gr.EPI_OUT_OP, gr.ACT_QUICK_GELU, True, False), (gr.EPI_OUT_OP, gr.ACT_GELU_ERF, False, False), (gr.EPI_SWIGLU_OP, 0, False, False),
        (gr.EPI_SWIGLU_OP, 0, True, False)]
ROPE = [(gr.EPI_ROPE_OP, 0, False, False), (gr.EPI_ROPE_OP, 0, True, False)]
LO8 = [(gr.EPI_OUT_OP, 0, True, True), (gr.EPI_OUT_OP, gr.ACT_GELU_ERF, True, True)]


def _epis(kform):
    return EPIS + (ROPE if kform == "16bit" else []) + (LO8 if kform.startswith("e4m3") else [])


def _problem(kform, fam, dt, M, N, K, k2, e, seed=0, kernel="product"):
    epi, act, bias, lo8 = e
    return gr.make_problem(kform, fam, dt, M, N, K, epi=epi, act=act, bias=bias, k2=k2, lo8_out=lo8, seed=seed, kernel=kernel,
                           rope_cols=256 if epi == gr.EPI_ROPE_OP else 0, rope_hd=64 if epi == gr.EPI_ROPE_OP else 0)


def _families(kform):
    return [f for f in gr.FAMILIES if not (f == "exact" and kform == "ext_split_blo")]      # (B_lo: the dropped t_lo x B_lo cannot vanish)


@pytest.mark.parametrize("kform,k2", [("16bit", 0), ("split", 0), ("ext", 64), ("ext_split", 64), ("ext_split_blo", 128), ("e4m3", 0),
                                      ("e4m3_third", 0), ("w8a8", 0)])
def test_reference_is_the_plain_fp64_operation(kform, k2):
    """Every epilogue and K-loop form: the segment-wise reference equals the operation written out at once from the uploaded tensors."""
    for fam in _families(kform):
        for dt in ("bf16", "f16"):
            for e in _epis(kform):
                P = _problem(kform, fam, dt, 70, 384, 256, k2, e, seed=1)
                y, _ = gr.reference(P, want_bound=False)
                want = gr.naive(P)
                assert (y - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item()), (kform, fam, dt, e)
                y2 = torch.cat([gr.reference(P, want_bound=False, rows=slice(a, min(a + 32, 70)))[0] for a in range(0, 70, 32)])
                assert (y - y2).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())      # the row-chunked form of the large-M cases


EXACT_FORM_K = [x for x in gr.FORM_K if x[0] != "ext_split_blo"]          # (no exact family with B_lo, see _families)


@pytest.mark.parametrize("kform,K,k2", EXACT_FORM_K, ids=[f"{f}-K{K}-k{k2}" for f, K, k2 in EXACT_FORM_K])
def test_exact_family_is_exact(kform, K, k2):
    """The precondition holds (make_problem asserts it) and fp32 sums in three orders equal the fp64 one; the hi / lo halves restore
    A; the block-scaled e4m3 encodings of the residuals and of the weights are exact under e8m0_of_amax's scales."""
    M, N = (34, 40) if K > 4096 else (130, 136)
    for dt in ("bf16", "f16"):
        P = gr.make_problem(kform, "exact", dt, M, N, K, epi=gr.EPI_OUT_F32, bias=True, k2=k2, seed=2)
        y, _ = gr.reference(P, want_bound=False)
        b32 = P.bias
        fwd = torch.zeros(M, N)
        for _, a, w, _ in P.segs:
            for k0 in range(0, a.shape[1], 64):
                fwd = fwd + a[:, k0:k0 + 64].float() @ w[:, k0:k0 + 64].float().T
        bwd = torch.zeros(M, N)
        for _, a, w, _ in reversed(P.segs):
            for k0 in reversed(range(0, a.shape[1], 16)):
                bwd = bwd + a[:, k0:k0 + 16].float() @ w[:, k0:k0 + 16].float().T
        whole = sum(a.float() @ w.float().T for _, a, w, _ in P.segs)
        sc = (P.ascale[:, None] * P.wscale[None, :]) if kform == "w8a8" else 1.0
        for got in (fwd, bwd, whole):
            assert torch.equal(((got * sc) + b32).double(), y), (kform, K, dt)
        assert torch.equal(gr.emulate_fp32(P), y)
        if kform in ("split", "e4m3", "e4m3_third", "ext_split"):
            hi, lo = P.A[:, :K].double(), P.A[:, K:].double()
            assert torch.equal(gr.split((hi + lo).float(), gr.TDT[dt])[0].double(), hi)
        if kform.startswith("e4m3"):
            lo = P.A[:, K:].double()
            E = gr.block_E(lo)
            sc_ = lo * torch.exp2(127 - E.double())
            assert torch.equal(sc_.float().to(torch.float8_e4m3fn).double(), sc_)
            assert len(torch.unique(E)) >= 5 or K < 256                    # several distinct block scales occur
            Wd = P.W.double()
            ws = Wd * torch.exp2(127 - gr.e8m0_of_amax(Wd.abs().amax()).double())
            assert torch.equal(ws.float().to(torch.float8_e4m3fn).double(), ws)
        if kform == "e4m3_third":
            hi, wl = P.A[:, :K].double(), P.Wlo.double()
            hs = hi * torch.exp2(127 - gr.e8m0_of_amax(hi.abs().amax(dim=1, keepdim=True)).double())
            assert torch.equal(hs.float().to(torch.float8_e4m3fn).double(), hs)
            wls = wl * torch.exp2(127 - gr.e8m0_of_amax(wl.abs().amax()).double())
            assert torch.equal(wls.float().to(torch.float8_e4m3fn).double(), wls) and bool((wl != 0).any())
            assert float((P.A[:, K:].double().abs() @ wl.abs().T).max()) == 0.0      # the dropped lo x lo term vanishes


def test_e4m3_quantisation_bound_holds_for_torch_rounding():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(64, 512, generator=g) * torch.exp2(torch.randint(-20, 4, (64, 1), generator=g).float())
    x[:, ::7] *= 2.0 ** -9                                                     # elements far below their block's maximum (e4m3 subnormals)
    E = gr.block_E(x.double())
    dec = (x.double() * torch.exp2(127 - E.double())).float().to(torch.float8_e4m3fn).double() * torch.exp2(E.double() - 127)
    assert bool(((dec - x.double()).abs() <= gr.qerr(x.double(), E)).all())


def test_bound_has_the_scale_of_its_rounding_model():
    M, N, K = 130, 384, 512
    for dt in ("bf16", "f16"):
        u = gr.U[dt]
        P1 = _problem("16bit", "normal", dt, M, N, K, 0, EPIS[2], seed=3)
        y1, b1 = gr.reference(P1)
        assert bool((b1 >= u * y1.abs()).all())
        aw = P1.segs[0][1].abs() @ P1.segs[0][2].abs().T
        assert bool((b1 <= u * y1.abs() + 2.0 ** -25 + 2.0 ** -16 * aw).all())          # single pass ~ u |y|: the fp32 terms stay below 2^-16 |A||W|^T
        # split and e4m3 bounds as a fraction of the single-pass operand rounding u |A||W|^T
        for kform, frac in (("split", 2.0 ** -6), ("e4m3", 2.0 ** -3)):
            P2 = _problem(kform, "normal", dt, M, N, K, 0, EPIS[0], seed=3)
            _, b2 = gr.reference(P2)
            aw2 = (P2.segs[0][1] + P2.segs[1][1]).abs() @ P2.segs[0][2].abs().T
            r = (b2 / (u * aw2)).max().item()
            print(f"[bound scale {dt} {kform}] bound / (u |A||W|^T) max {r:.3g} (stated fraction {frac:.3g})")
            assert r < frac, (dt, kform, r)
    # an fp32 emulation that accumulates K-tile by K-tile stays under the bound on every family and form without one-byte operands
    for kform, k2 in (("16bit", 0), ("split", 0), ("ext_split_blo", 64), ("w8a8", 0)):
        for fam in _families(kform):
            for e in _epis(kform):
                for kernel in ("product", "plain"):
                    if kernel == "plain" and (kform not in ("16bit", "split") or e[0] == gr.EPI_ROPE_OP):
                        continue
                    P = _problem(kform, fam, "f16", 70, 384, 704, k2, e, seed=5, kernel=kernel)
                    y, b = gr.reference(P)
                    r = gr.max_ratio((gr.emulate_fp32(P) - y).abs(), b)
                    assert r <= 1.0, (kform, fam, e, kernel, r)


def _exact_leg(P, mut):
    """A mutant on the `exact` family: True when at least one output bit differs (fp32 and un-activated operand outputs) or the value
    leaves the accumulation-free bound (activated outputs)."""
    y, b = gr.reference(P)
    m, _ = gr.reference(P, mutant=mut, want_bound=False)
    if P.epi in (gr.EPI_OUT_F32, gr.EPI_RESADD_F32) or (P.epi == gr.EPI_OUT_OP and P.act == 0 and not P.lo8_out):
        if mut == "out_lo_zero":
            return bool((gr.expected_bits(P, y)[1] != 0).any())
        return any(not torch.equal(a, c) for a, c in zip(gr.expected_bits(P, y), gr.expected_bits(P, m)))
    return gr.max_ratio((m - y).abs(), b) > 1.0


@pytest.mark.parametrize("kform,K,k2", gr.FORM_K, ids=[f"{f}-K{K}-k{k2}" for f, K, k2 in gr.FORM_K])
def test_every_mutant_is_caught(kform, K, k2):
    """At every (form, K) of the GPU file: every structural mutant changes at least one bit on `exact`, and every numerical mutant lands
    above the bound on a real-valued family; the ratios of the structural ones on the real-valued families are printed (the rounding
    model cannot separate all of them at every K -- that is what `exact` is for)."""
    big = K > 4096
    M, N = (258, 384)
    epis = [EPIS[0], EPIS[2]] if big else _epis(kform)
    fams = _families(kform)
    exact_hit, real_best, seen = {}, {}, set()
    for e in epis:
        for fam in fams:
            P = _problem(kform, fam, "f16", M, N, K, k2, e, seed=6)
            if fam != "exact":
                y, b = gr.reference(P)
            for mut in gr.MUTANTS:
                if not gr.applicable(mut, P):
                    continue
                seen.add(mut)
                if fam == "exact":
                    exact_hit[mut] = exact_hit.get(mut, False) or _exact_leg(P, mut)
                else:
                    m, _ = gr.reference(P, mutant=mut, want_bound=False)
                    real_best[mut] = max(real_best.get(mut, 0.0), gr.max_ratio((m - y).abs(), b))
    for mut in sorted(seen):
        ex, rr = exact_hit.get(mut), real_best.get(mut, 0.0)
        leg = "+".join(n for n, ok in (("exact", ex), ("bound", rr > 1.0)) if ok) or "NONE"
        print(f"[{kform} K={K} k2={k2}] {mut}: exact leg {ex}, best real-valued err/bound {rr:.3g} -> caught by {leg}")
        if mut in gr.NUMERICAL_MUTANTS:
            assert rr > 1.0, (kform, K, mut, rr)
        elif "exact" in fams:
            assert ex, (kform, K, mut)
        else:
            assert rr > 1.0, (kform, K, mut, rr)


def test_dispatch_table_covers_every_launchable_instantiation():
    gemm = open(os.path.join(CSRC, "gemm.hip")).read()
    gemm8 = open(os.path.join(CSRC, "gemm8.hip")).read()
    narrow = open(os.path.join(CSRC, "gemm8_narrow.hip")).read()
    assert "#include \"gemm8.hip\"" in narrow and "launch8<" not in narrow.replace("#include", "")      # the narrow unit adds no sites of its own
    prod, excl = gr.launch_sites(gemm, gemm8)
    table = {gr.instantiation(c) for c in gr.all_cells()}
    assert not (table & gr.engine_only())
    assert table | gr.engine_only() == prod, (sorted(table - prod), sorted(prod - table - gr.engine_only()))
    assert not (table & {x for x in excl if x[3] == 0 and x[6] != 3})
    assert all(x[3] != 0 or x[6] == 3 for x in excl)                              # excluded = diagnostic (DBG) or FP6 A/B instantiations
    c = gr.source_constants(gemm8)
    assert (c["ring_product"], c["ring_other"]) == (gr.RING_SLOTS["product"], gr.RING_SLOTS["other"])
    assert c["gm"] == gr.GM_DEFAULT and (c["narrow_cost"], c["narrow_gain"]) == (gr.NARROW_COST, gr.NARROW_GAIN)
    assert c["dynamic_factor"] == 4 and c["band_rule"]
    assert "aligned && p.N >= 256 && p.K >= 128) ? 6 : 0" in gemm and "E == EPI_OUT_OP && p.N <= 128) return 2" in gemm8
    # the restated conditions at their edges
    assert gr.pick_tile(256, 128, -1) == 6 and gr.pick_tile(248, 128, -1) == 0 and gr.pick_tile(256, 64, -1) == 0
    assert gr.pick_tile(260, 128, -1) == 0 and gr.pick_tile(512, 512, -1, aligned=False) == 0 and gr.pick_tile(64, 64, 6) == 6
    assert gr.narrow_choice(1, 768, gr.EPI_OUT_F32, 256) == 1 and gr.narrow_choice(300, 128, gr.EPI_OUT_OP, 256) == 2
    assert gr.narrow_choice(300, 128, gr.EPI_OUT_F32, 256) == 1 and gr.narrow_choice(300, 128, gr.EPI_OUT_OP, 256, force=0) == 0
    assert gr.narrow_choice(256 * 256, 256, gr.EPI_OUT_F32, 256) == 0 and gr.narrow_choice(256 * 256, 256, gr.EPI_OUT_F32, 256, force=1) == 1
    assert gr.walk("product", 513, 520, (256, 256), 256) == "static" and gr.walk("plain", 513, 520, (128, 128), 256) == "one_tile"
    assert gr.walk("product", 8200, 8192, (256, 256), 256) == "dynamic" and gr.walk("product", 16643, 4096, (256, 256), 256) == "dynamic_bands"
    assert gr.walk("product", 16643, 4096, (256, 256), 256, bandchunk=False) == "dynamic"
    assert gr.walk("product", 15361, 4608, (256, 256), 256) == "dynamic_bands"       # 61 row tiles = 16 bands: chunks on from here
    assert gr.walk("product", 15360, 4608, (256, 256), 256) == "dynamic"             # 60 row tiles = 15 bands
    assert gr.walk("product", 16643, 4096, (256, 256), 304) == "static"              # 1056 tiles < 4 x 304
    assert {k for k, _ in gr.ALL_WALKS} == {c[0] for c in gr.all_cells()}
