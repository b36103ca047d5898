"""CPU checks of tests/helpers/attention_ref.py, the fp64 reference and per-element bound the attention kernel tests assert against:
the chunked reference is the plain softmax, every wrong-rule mutant of the reference lands above the bound somewhere on every input
family (so the GPU assertions have teeth), and the dispatch table covers every instantiation launch_one can reach."""
import os

import pytest
import torch

from helpers import attention_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTN_SRC = os.path.join(ROOT, "llava-reward_amd", "csrc", "attention.hip")

FORMS_DT = [("bf16", False, torch.bfloat16), ("f16", False, torch.float16), ("bf16", True, torch.bfloat16), ("f16", True, torch.float16)]


def _mask(B, S, rows):
    m = torch.ones(B, S, dtype=torch.int64)
    for b, spans in enumerate(rows):
        for a, e in spans:
            m[b, a:e] = 0
    return m


# (name, hd, causal, B, S, H, Hkv, mask spans per row or None, segments or None); shapes of tests/test_gpu_attention.py, the smaller ones
CASES = [
    ("causal96", 96, True, 2, 300, 2, 1, [[(0, 37)], [(0, 100), (150, 170)]], None),
    ("dense64", 64, False, 1, 200, 1, 1, [[(70, 90), (120, 125)]], None),
    ("ragged96", 96, False, 1, 255, 1, 1, None, [0, 1, 128, 255]),
    ("causal128_pp", 128, True, 1, 1025, 1, 1, [[(0, 1001)]], None),
]


def _operands(fam, case, dt, sp, tdt):
    name, hd, causal, B, S, H, Hkv, spans, segs = case
    scale = (80 ** -0.5) if segs is not None else hd ** -0.5
    mask = _mask(B, S, spans) if spans is not None else None
    q, k, v = ar.make_inputs(fam, B, S, H, Hkv, hd, scale=scale, mask=mask, segments=segs, seed=5)
    if sp:
        parts = [ar.split(x, tdt) for x in (q, k, v)]
        vals = [(h.double() + l.double()) for h, l in parts]
        lo = [l.double() for _, l in parts]
    else:
        vals = [x.to(tdt).double() for x in (q, k, v)]
        lo = None
    return vals, lo, scale, mask


def test_chunked_reference_is_the_plain_softmax():
    for case in CASES[:3]:
        name, hd, causal, B, S, H, Hkv, spans, segs = case
        (q, k, v), _, scale, mask = _operands("normal", case, "bf16", False, torch.bfloat16)
        got, _ = ar.reference(q, k, v, scale=scale, causal=causal, mask=mask, segments=segs, kv_group=H // Hkv, want_bound=False, chunk=64)
        want = ar.naive(q, k, v, scale=scale, causal=causal, mask=mask, segments=segs, kv_group=H // Hkv)
        assert (got - want).abs().max().item() < 1e-12, name
    # GQA (repeat_interleave over kv_group) and a row with no visible key (exact zeros)
    B, S, H, Hkv, hd = 1, 70, 4, 2, 64
    q, k, v = ar.make_inputs("normal", B, S, H, Hkv, hd, scale=0.125, seed=1)
    mask = torch.ones(B, S, dtype=torch.int64)
    mask[0, :S] = 0
    got, bnd = ar.reference(q, k, v, scale=0.125, causal=True, mask=mask, kv_group=2, dtype="f16", chunk=16)
    assert torch.equal(got, torch.zeros_like(got)) and torch.equal(bnd, torch.zeros_like(bnd))
    got, _ = ar.reference(q, k, v, scale=0.125, causal=True, kv_group=2, want_bound=False, chunk=16)
    want = ar.naive(q, k, v, scale=0.125, causal=True, kv_group=2)
    assert (got - want).abs().max().item() < 1e-12


def test_bound_has_the_rounding_model_scale():
    """The single-pass bound is ~u (P|V| + |o|) and the split bound is orders of magnitude below it (u^2 + fp32 terms)."""
    case = CASES[0]
    for dt, tdt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        (q, k, v), _, scale, mask = _operands("normal", case, dt, False, tdt)
        o, b1 = ar.reference(q, k, v, scale=scale, causal=True, mask=mask, kv_group=2, dtype=dt)
        (q, k, v), lo, _, _ = _operands("normal", case, dt, True, tdt)
        _, b2 = ar.reference(q, k, v, scale=scale, causal=True, mask=mask, kv_group=2, dtype=dt, split=True, lo=lo)
        valid = b1 > 0
        assert (b1[valid] >= ar.U[dt] * o.abs()[valid]).all()
        assert (b1[valid] < 4 * ar.U[dt] * (v.abs().max() + o.abs()[valid])).all()
        assert (b2[valid] < (0.1 if dt == "bf16" else 0.5) * b1[valid]).all()


def _applicable(mutant, case):
    name, hd, causal, B, S, H, Hkv, spans, segs = case
    if mutant in ("diag_plus1", "diag_minus1", "wave_causal"):
        return causal
    if mutant == "kmin_round_up":
        return causal and spans is not None and any(s[0][0] == 0 and s[0][1] % 64 for s in spans)
    if mutant == "unmask_one":
        return spans is not None
    return True


@pytest.mark.parametrize("fam", ar.FAMILIES)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_mutant_exceeds_the_bound(fam, case):
    name, hd, causal, B, S, H, Hkv, spans, segs = case
    if fam == "poison" and spans is None and segs is None:
        pytest.skip("no masked keys to poison")      # (not reached: every case has a mask or segments)
    for dt, sp, tdt in FORMS_DT:
        (q, k, v), lo, scale, mask = _operands(fam, case, dt, sp, tdt)
        kw = dict(scale=scale, causal=causal, mask=mask, segments=segs, kv_group=H // Hkv)
        ref, bnd = ar.reference(q, k, v, dtype=dt, split=sp, lo=lo, **kw)
        for mut in ar.MUTANTS:
            if not _applicable(mut, case):
                continue
            m, _ = ar.reference(q, k, v, want_bound=False, mutant=mut, **kw)
            r = ar.max_ratio((m - ref).abs(), bnd)
            print(f"[{name} {fam} {dt}{'x2' if sp else ''}] {mut}: max err/bound {r:.3g}")
            assert r > 1.0, (name, fam, dt, sp, mut, r)


def test_dispatch_table_covers_every_reachable_instantiation():
    src = open(ATTN_SRC).read()
    assert ar.attention_forms(src) == set(ar.FORMS)
    assert {c for row in ar.TABLE.values() for c in row} == ar.launch_sites(src)
    # the table restates dispatch() (launch_one as data) at every band edge, with and without the ping-pong schedule
    seen = set()
    for hd, causal in ar.FORMS:
        for sp in (False, True):
            for S in (1, 128, 129, 1023, 1024, 8192):
                inst = ar.dispatch(hd, causal, sp, S)
                assert inst == ar.TABLE[ar.band(sp, S)][ar.FORMS.index((hd, causal))], (hd, causal, sp, S)
                seen.add((hd, causal) + inst + (False,))
                off = ar.dispatch(hd, causal, sp, S, pingpong=False)
                assert not off[2]
                seen.add((hd, causal) + off + (False,))
        if not causal:
            for sp in (False, True):
                seen.add((hd, causal) + ar.dispatch(hd, causal, sp, 5120, ragged=True) + (True,))
    assert seen == ar.all_cells()
    assert len({c[:5] for c in ar.all_cells()}) == 22            # x 2 operand types = the 44 instantiations of attn_kernel
