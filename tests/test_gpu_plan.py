"""The kernels that decide which position a token has, which image row it reads and which rotation its q and k get, each on its own
(lr_op_token_plan, lr_op_slot_check, lr_op_prefix_header, lr_op_embed, lr_op_rope_table, lr_op_rope_split, lr_op_qwen_plan, lr_op_mrope_table,
lr_op_vit_rope_table, lr_op_qwen_ca_vec) against the plain references of tests/helpers/plan_ref.py: integer outputs and copies exactly,
rope_split bit for bit, tables within the trig bound.  The qwen plan is also compared with transformers' own get_rope_index as recorded in
golden/plan_qwen_rope_index.json.  Inputs are followed by poison that would change the result if read (image-slot ids, flipped mask
values, positions, table rows); outputs sit between sentinel guard rows (with sentinel gap columns where the kernel takes a leading
dimension), and every launch checks that nothing else was written.  Refusals are tested through LR_EINVAL of calls that launch nothing.
Every table case prints max err / bound; the last test prints the largest per kernel (the measured trig accuracy)."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import plan_ref as pr
from helpers.guards import DEV, GR, Out, P, _in, _stream
from llava_reward_amd import _lib as L

pytestmark = pytest.mark.gpu

CODE = {"bf16": L.LR_DT_BF16, "f16": L.LR_DT_F16}
LR_EINVAL = 1                  # include/llava_reward_hip.h
NAN = float("nan")
RATIOS = {}                    # table kernel -> largest err / bound seen (printed by the last test)
I32 = torch.int32


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return L.load()


@pytest.fixture(scope="module")
def qwen_golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_qwen_rope_index.json")) as f:
        return json.load(f)["cases"]


def _ints(a, fill, dtype=torch.int64):
    """An integer array at the head of an allocation whose other rows hold `fill`."""
    return _in(torch.as_tensor(np.asarray(a)).to(dtype), fill=fill)


def _vec(a, fill, dtype=I32, extra=16):
    """A flat integer / float array followed by `extra` elements of `fill`."""
    t = torch.as_tensor(np.asarray(a)).to(dtype).flatten()
    buf = torch.full((t.numel() + extra,), fill, dtype=dtype, device=DEV)
    buf[:t.numel()] = t.to(DEV)
    return buf


def _iout(rows, cols, ld=None):
    return Out(rows, cols, ld=ld)                                 # int32 words between int32 sentinels: .all is the integer view


def _ibody(out):
    return out.all[GR:GR + out.rows, :out.cols].cpu().numpy().astype(np.int64)


def _bits16(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------------------------------
# token plan, slot check, prefix header
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pr.token_plan_cases(), ids=lambda c: f"S{c[0]}-{c[1]}-{'_'.join(c[2])}")
def test_token_plan(lib, case):
    Pt = pr.make_token_plan(case)
    B, S = Pt.B, Pt.S
    slot_id = Pt.image_token_id if Pt.image_token_id >= 0 else -1
    ids = _ints(Pt.ids, slot_id)                                  # behind the rows: image slots
    mask = None if Pt.mask is None else _ints(Pt.mask, 1 - int(Pt.mask[-1, -1]))      # behind the rows: the opposite of the last token's value
    voff = _vec(Pt.voff, 10 ** 6)
    img_base = None if Pt.img_base is None else _vec([Pt.img_base], 10 ** 5)
    pos, img_row, tstat = _iout(B, S), _iout(B, S), _iout(B, 4)
    rc = lib.lr_op_token_plan(P(ids), P(mask), B, S, P(voff), img_row.ptr, pos.ptr, tstat.ptr, Pt.image_token_id, Pt.pos_arange, Pt.pos_base,
                              P(img_base), Pt.vs, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    for o, what in ((pos, "pos"), (img_row, "img_row"), (tstat, "tstat")):
        o.check(f"token_plan {what}")
    wpos, wrow, wstat = pr.token_plan_run(Pt)
    assert np.array_equal(_ibody(pos), wpos), "pos"
    assert np.array_equal(_ibody(img_row), wrow), "img_row"
    assert np.array_equal(_ibody(tstat), wstat), ("tstat", _ibody(tstat).tolist(), wstat.tolist())


@pytest.mark.parametrize("B,d", [(3, 2), (16, 4), (13, 7)], ids=["Bd6", "Bd64", "Bd91"])
@pytest.mark.parametrize("vs", [1, 0])
def test_slot_check(lib, B, d, vs):
    g = np.random.default_rng(B * 10 + d)
    counts = g.integers(0, 9, B)
    voff = np.concatenate([[4], 4 + np.cumsum(counts)])
    tstat = g.integers(0, 50, (B, 4))
    cap = counts if vs == 1 else np.full(B, counts[0])
    tstat[:, 2] = cap
    tstat[1::3, 2] += 1                                           # one slot too many
    tstat[2::5, 2] = np.maximum(tstat[2::5, 2] - 1, 0) + (tstat[2::5, 2] == 0) * 2      # one too few (or two too many where there are none)
    rewards = g.standard_normal((B, d)).astype(np.float32)
    rewards[0, 0] = -0.0
    want = pr.slot_check_ref(tstat, voff, rewards, vs)
    assert np.isnan(want).any() and not np.isnan(want).all()
    out = Out(B, d)
    out.body.copy_(torch.from_numpy(rewards))
    tstat_d, voff_d = _vec(tstat, 10 ** 6), _vec(voff if vs else voff[:2], 10 ** 6)       # (named: both live until the kernel has run)
    rc = lib.lr_op_slot_check(P(tstat_d), P(voff_d), out.ptr, B, d, vs, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    out.check("slot_check")
    got = out.body.cpu().numpy()
    bad = np.isnan(want)
    assert np.isnan(got[bad]).all() and np.array_equal(got[~bad].view(np.int32), want[~bad].view(np.int32)), "rows that match keep their exact bits"


def test_prefix_header(lib):
    hdr = _iout(1, 3, ld=8)
    tstat = _vec([9, 0, 1733, 40], 10 ** 6)
    rc = lib.lr_op_prefix_header(P(tstat), 1921, hdr.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    hdr.check("prefix_header")
    assert _ibody(hdr).tolist() == [[0, 1921, 1733]]


# ---------------------------------------------------------------------------------------------------------------------------------------
# embedding
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pr.embed_cases(), ids=lambda c: f"{c[0]}x{c[1]}-{'ev' if c[2] else 'noev'}")
def test_embed(lib, case):
    Pe = pr.make_embed(*case)
    ids = _vec(Pe.ids, 1, dtype=torch.int64)
    img_row = _vec(Pe.img_row, 0)
    wte = _in(Pe.wte.view(torch.int16), fill=int(torch.tensor(3.0e4).bfloat16().view(torch.int16)))           # row `vocab` and the rows behind: poison
    ev = _in(Pe.ev, fill=NAN) if Pe.ev is not None else None
    out = Out(Pe.rows, Pe.D)
    rc = lib.lr_op_embed(P(ids), P(img_row), P(wte), P(ev), out.ptr, Pe.rows, Pe.D, Pe.vocab, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    out.check("embed")
    want = pr.embed_ref(Pe.ids, Pe.img_row, Pe.wte, Pe.ev, Pe.vocab)
    assert torch.equal(out.body.cpu().view(I32), want.view(I32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# rope_split, fused against fallback
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rope_split_launch(lib, qkv_dev, cs_dev, rows, rope_cols, v_cols, hd, dt, prec):
    n = rope_cols + v_cols
    out = Out(rows, n << prec, dtype=pr.TDT[dt])
    rc = lib.lr_op_rope_split(P(qkv_dev), P(cs_dev), out.ptr, rows, rope_cols, v_cols, hd, CODE[dt], prec, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, rows, rope_cols, v_cols, hd, dt, prec)
    out.check("rope_split")
    return out


@pytest.mark.parametrize("case", pr.rope_split_cases(), ids=lambda c: "-".join(map(str, c)))
def test_rope_split_bit_for_bit(lib, case):
    Ps = pr.make_rope_split(*case)
    n = Ps.rope_cols + Ps.v_cols
    qkv, cs = _in(Ps.qkv), _in(Ps.cs.reshape(Ps.rows, -1), fill=NAN)
    for dt in ("bf16", "f16"):
        single = None
        for prec in (0, 1):
            out = _rope_split_launch(lib, qkv, cs, Ps.rows, Ps.rope_cols, Ps.v_cols, Ps.hd, dt, prec)
            want = _bits16(pr.rope_split_ref(Ps.qkv, Ps.cs, Ps.rope_cols, Ps.v_cols, Ps.hd, dt, prec))
            got = _bits16(out.body.cpu())
            parts = {"hi rotated": (0, Ps.rope_cols), "hi v": (Ps.rope_cols, n)}
            if prec:
                parts.update({"lo rotated": (n, n + Ps.rope_cols), "lo v": (n + Ps.rope_cols, 2 * n)})
            for what, (a, b) in parts.items():
                assert torch.equal(got[:, a:b], want[:, a:b]), (case, dt, prec, what, int((got[:, a:b] != want[:, a:b]).sum()))
            if prec == 0:
                single = got
            else:
                assert torch.equal(got[:, :n], single), "the hi half differs from the single-operand output"


def test_rope_split_refusals_launch_nothing(lib):
    x = _in(torch.zeros(2, 64))
    out = Out(2, 128, dtype=torch.float16)
    for hd, rope_cols, v_cols in ((12, 24, 0), (8, 20, 0), (8, 16, 6)):
        assert pr.rope_split_refused(hd, rope_cols, v_cols)
        assert lib.lr_op_rope_split(P(x), P(x), out.ptr, 2, rope_cols, v_cols, hd, CODE["f16"], 1, _stream()) == LR_EINVAL
    torch.cuda.synchronize()
    assert out.untouched()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_fused_rope_and_fallback_give_the_same_bits(lib, dt):
    """The engine takes the fused epilogue or fp32 projection + rope_split by problem size (engine.h qkv_rope): an exact-integer
    projection through both, at the smallest M and N at which the deep kernel runs, must give the same bits -- else a reward would change
    with the batch size."""
    M, D, hd, K = 256, 384, 96, 128
    N, half = 3 * D, hd // 2
    tdt = pr.TDT[dt]
    g = torch.Generator().manual_seed(77)
    A = torch.randint(-4, 5, (M, K), generator=g).float()
    W = torch.randint(-1, 2, (N, K), generator=g).float()
    ang = torch.rand(M, half, generator=g) * 6.3
    cs = torch.stack([torch.cos(ang) * 1.19, torch.sin(ang) * 1.19], dim=-1).contiguous()
    y = A @ W.t()                                                # |sums| <= 512: exact in fp32 in any order
    assert bool((y == y.round()).all())
    Ad, Wd, csd = _in(A.to(tdt)), _in(W.to(tdt)), _in(cs.reshape(M, -1), fill=NAN)
    fused = Out(M, N, dtype=tdt)
    assert lib.lr_op_gemm_rope(P(Ad), P(Wd), fused.ptr, None, P(csd), M, N, K, 2 * D, hd, CODE[dt], -1, _stream()) == 0
    y32 = Out(M, N)
    assert lib.lr_op_gemm_bt(P(Ad), P(Wd), y32.ptr, None, M, N, K, K, K, N, L.EPI_OUT_F32, L.ACT_NONE, CODE[dt], -1, _stream()) == 0
    torch.cuda.synchronize()
    fused.check("gemm_rope")
    y32.check("gemm_bt")
    assert torch.equal(y32.body.cpu(), y), "the fp32 projection is not the exact integer result"
    y32d = y32.body.contiguous()
    fallback = _rope_split_launch(lib, y32d, csd, M, 2 * D, D, hd, dt, 0)
    assert torch.equal(_bits16(fused.body), _bits16(fallback.body)), int((_bits16(fused.body) != _bits16(fallback.body)).sum())
    assert torch.equal(_bits16(fallback.body.cpu()), _bits16(pr.rope_split_ref(y, cs, 2 * D, D, hd, dt, 0)))


# ---------------------------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------------------------
def _table_compare(key, label, out, y, E):
    got = out.body.cpu().view(y.shape)
    worst = pr.table_ratio(got, y, E)
    err = (got.double() - y).abs()
    print(f"[{key} {label}] max err/bound {worst:.3g}  max err {err.max().item():.3g}")
    if worst > 1.0:
        r = torch.where(E > 0, err / E.clamp_min(1e-300), (err > 0).double() * 1e300)
        i = int(r.argmax())
        print(f"  worst element {i} of shape {tuple(y.shape)}: got {got.flatten()[i].item()!r} want {y.flatten()[i].item()!r} bound {E.flatten()[i].item():.3g}")
    assert worst <= 1.0, (key, label, worst)
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
    return got


def _rope_table_launch(lib, Pt):
    rows = Pt.B * Pt.S
    pos = _vec(Pt.pos, 777)                                       # behind the rows: other positions
    inv_s, inv_l = _vec(Pt.inv_s, NAN, dtype=torch.float32), _vec(Pt.inv_l, NAN, dtype=torch.float32)
    out = Out(rows, 2 * Pt.half)
    rc = lib.lr_op_rope_table(P(pos), None, Pt.B, Pt.S, P(inv_s), P(inv_l), Pt.scaling, Pt.orig_max, Pt.half, out.ptr, Pt.rot, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    out.check("rope_table")
    return out


@pytest.mark.parametrize("case", pr.rope_table_cases(), ids=lambda c: "-".join(map(str, c)))
def test_rope_table(lib, case):
    Pt = pr.make_rope_table(*case)
    out = _rope_table_launch(lib, Pt)
    y, E = pr.rope_table_run(Pt)
    got = _table_compare("rope_table", str(case), out, y, E)
    other = pr.rope_table_ref(Pt.pos, Pt.S, Pt.inv_l, Pt.inv_s, Pt.scaling, Pt.orig_max, Pt.rot)      # the other factor set leaves the bound
    assert pr.table_ratio(got, *other) > 1.0
    zero = torch.from_numpy(Pt.pos == 0)
    assert torch.equal(got[zero, :, 0], torch.full_like(got[zero, :, 0], Pt.scaling)) and bool((got[zero, :, 1] == 0).all())


def test_rope_table_feeds_rope_split(lib):
    """Composite: the table the kernel produced goes into rope_split; the output is the reference rotation by THAT table, bit for bit."""
    Pt = pr.make_rope_table(48, 3, 4, 9, "su")
    tab = _rope_table_launch(lib, Pt)
    rows, hd = 12, 96
    Ps = pr.make_rope_split(rows, hd, 2 * hd, 4, "normal", seed=3)
    cs_dev = _in(tab.body, fill=NAN)
    cs = tab.body.cpu().view(rows, hd // 2, 2)
    for dt in ("bf16", "f16"):
        qkv = _in(Ps.qkv)
        out = _rope_split_launch(lib, qkv, cs_dev, rows, 2 * hd, 4, hd, dt, 1)
        assert torch.equal(_bits16(out.body.cpu()), _bits16(pr.rope_split_ref(Ps.qkv, cs, 2 * hd, 4, hd, dt, 1)))


@pytest.mark.parametrize("case", pr.mrope_cases(), ids=lambda c: "-".join(map(str, c)))
def test_mrope_table(lib, case):
    Pm = pr.make_mrope(*case)
    out = Out(Pm.rows, 2 * Pm.half)
    pos3, inv = _vec(Pm.pos3, 777), _vec(Pm.inv, NAN, dtype=torch.float32)
    rc = lib.lr_op_mrope_table(P(pos3), Pm.rows, P(inv), Pm.s0, Pm.s1, Pm.half, out.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    out.check("mrope_table")
    _table_compare("mrope_table", str(case), out, *pr.mrope_table_ref(Pm.pos3, Pm.inv, Pm.s0, Pm.s1))


@pytest.mark.parametrize("case", pr.vit_cases(), ids=lambda c: "-".join(map(str, c)))
def test_vit_rope_table(lib, case):
    Pv = pr.make_vit(*case)
    out = Out(Pv.rows, 2 * Pv.half_pad)
    hw, inv = _vec(Pv.hw, 777), _vec(Pv.inv, NAN, dtype=torch.float32)
    rc = lib.lr_op_vit_rope_table(P(hw), Pv.rows, P(inv), Pv.quarter, Pv.half_pad, out.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    out.check("vit_rope_table")
    got = _table_compare("vit_rope_table", str(case), out, *pr.vit_rope_table_ref(Pv.hw, Pv.inv, Pv.quarter, Pv.half_pad))
    pad = got[:, 2 * Pv.quarter:]
    assert torch.equal(pad[..., 0], torch.ones_like(pad[..., 0])) and bool((pad[..., 1].view(I32) == 0).all()), "pad pairs are exactly (1, 0)"


# ---------------------------------------------------------------------------------------------------------------------------------------
# qwen plan, qwen_ca_vec
# ---------------------------------------------------------------------------------------------------------------------------------------
def _qwen_launch(lib, Pq):
    B, S = Pq.B, Pq.S
    ids = _ints(Pq.ids, pr.Q_IMAGE)                               # behind the rows: un-masked image slots
    mask = _ints(Pq.mask, 1)
    has = len(Pq.grid_thw) > 0
    imgs = _in(torch.from_numpy(Pq.imgs), fill=10 ** 6) if has else None
    s2r = _vec(Pq.slot2row, 10 ** 6) if has else None
    rstat, pos3, img_row = _iout(B, 4), _iout(3 * B, S), _iout(B, S)
    rc = lib.lr_op_qwen_plan(P(ids), P(mask), B, S, pr.Q_IMAGE, pr.Q_CA, P(imgs), len(Pq.grid_thw), P(s2r), Pq.n_slots if has else 0,
                             rstat.ptr, pos3.ptr, img_row.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    for o, what in ((rstat, "rstat"), (pos3, "pos3"), (img_row, "img_row")):
        o.check(f"qwen_plan {what}")
    return _ibody(pos3).reshape(3, B, S), _ibody(img_row), _ibody(rstat)


@pytest.mark.parametrize("name", list(pr.qwen_cases()))
def test_qwen_plan(lib, qwen_golden, name):
    Pq = pr.make_qwen(name)
    pos3, img_row, rstat = _qwen_launch(lib, Pq)
    wpos, wrow, wstat = pr.qwen_run(Pq)
    assert np.array_equal(pos3, wpos), "pos3 against the helper"
    assert np.array_equal(pos3, np.array(qwen_golden[name]["pos3"], np.int64)), "pos3 against get_rope_index"
    assert np.array_equal(img_row, wrow), "img_row"
    assert np.array_equal(rstat, wstat), ("rstat", rstat.tolist(), wstat.tolist())


@pytest.mark.parametrize("which", ["runs", "long"])
def test_qwen_plan_clamps_stay_in_range(lib, which):
    """More runs than images, and a run longer than its image: batches the host wrapper refuses.  The kernel's own clamps keep every index in
    range (the tables are followed by poison, the outputs by sentinels); the values are what it documents for clamping."""
    Pq = pr.make_qwen_clamped(which)
    pos3, img_row, rstat = _qwen_launch(lib, Pq)
    wpos, wrow, wstat = pr.qwen_run(Pq)
    assert int(img_row.max()) < Pq.n_slots and int(img_row.min()) >= -1
    assert np.array_equal(pos3, wpos) and np.array_equal(img_row, wrow) and np.array_equal(rstat, wstat)


@pytest.mark.parametrize("D", [4, 260])
def test_qwen_ca_vec(lib, D):
    B = 3
    rstat = np.array([[2, 0, 0, 0], [0, 3, 0, 0], [1, 0, 0, 0]])
    u = torch.randn(D, generator=torch.Generator().manual_seed(D))
    out = Out(B, D)
    rstat_d, u_d = _vec(rstat, 9), _vec(u, NAN, dtype=torch.float32)
    rc = lib.lr_op_qwen_ca_vec(P(rstat_d), P(u_d), B, D, out.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    out.check("qwen_ca_vec")
    want = torch.stack([torch.zeros(D), u, torch.zeros(D)])
    assert torch.equal(out.body.cpu().view(I32), want.view(I32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals, report
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_plan_refusals_launch_nothing(lib):
    st = _stream()
    ids = _ints(np.zeros((3, 8)), 0)
    mask = _ints(np.ones((3, 8)), 1)
    i32 = _vec(np.zeros(64), 0)
    f32 = _vec(np.ones(64), 1.0, dtype=torch.float32)
    wte = _in(torch.zeros(4, 8, dtype=torch.int16), fill=0)
    a, b, c = Out(3, 64), Out(3, 64), Out(3, 64)
    calls = [
        ("embed D % 4", lambda: lib.lr_op_embed(P(ids), P(i32), P(wte), None, a.ptr, 3, 6, 4, st)),
        ("embed vocab 0", lambda: lib.lr_op_embed(P(ids), P(i32), P(wte), None, a.ptr, 3, 8, 0, st)),
        ("token_plan S 0", lambda: lib.lr_op_token_plan(P(ids), P(mask), 3, 0, P(i32), a.ptr, b.ptr, c.ptr, -1, 0, 0, None, 1, st)),
        ("qwen_plan S 0", lambda: lib.lr_op_qwen_plan(P(ids), P(mask), 3, 0, 5, 6, None, 0, None, 0, a.ptr, b.ptr, c.ptr, st)),
        ("qwen_plan mask null", lambda: lib.lr_op_qwen_plan(P(ids), None, 3, 8, 5, 6, None, 0, None, 0, a.ptr, b.ptr, c.ptr, st)),
        ("qwen_plan n_images 0", lambda: lib.lr_op_qwen_plan(P(ids), P(mask), 3, 8, 5, 6, P(i32), 0, P(i32), 4, a.ptr, b.ptr, c.ptr, st)),
        ("qwen_plan n_slots 0", lambda: lib.lr_op_qwen_plan(P(ids), P(mask), 3, 8, 5, 6, P(i32), 1, P(i32), 0, a.ptr, b.ptr, c.ptr, st)),
        ("qwen_plan one table", lambda: lib.lr_op_qwen_plan(P(ids), P(mask), 3, 8, 5, 6, None, 0, P(i32), 0, a.ptr, b.ptr, c.ptr, st)),
        ("mrope s0 < 0", lambda: lib.lr_op_mrope_table(P(i32), 3, P(f32), -1, 2, 8, a.ptr, st)),
        ("mrope s1 < 0", lambda: lib.lr_op_mrope_table(P(i32), 3, P(f32), 2, -1, 8, a.ptr, st)),
        ("mrope s0 + s1 > half", lambda: lib.lr_op_mrope_table(P(i32), 3, P(f32), 5, 4, 8, a.ptr, st)),
        ("vit 2 quarter > half_pad", lambda: lib.lr_op_vit_rope_table(P(i32), 3, P(f32), 5, 8, a.ptr, st)),
    ]
    for what, call in calls:
        assert call() == LR_EINVAL, what
        torch.cuda.synchronize()
        assert a.untouched() and b.untouched() and c.untouched(), what


def test_zz_report_largest_ratio_per_table_kernel():
    print("\nlargest max err / bound per table kernel (TRIG_ULP = %d):" % pr.TRIG_ULP)
    for k in sorted(RATIOS):
        print(f"  {k:20s} {RATIOS[k]:.3g}")
    assert set(RATIOS) == {"rope_table", "mrope_table", "vit_rope_table"} and all(v <= 1.0 for v in RATIOS.values())
