"""The kernels that decide which pixel or CLIP feature lands in which operand row, each on its own (lr_op_im2col, lr_op_clip_embed,
lr_op_hd_gather, lr_op_clip_tokens, lr_op_llava_pack, lr_op_qwen_patch_gather) against the plain references of tests/helpers/vision_ref.py:
the copies bit for bit (values moved and rounded once to the operand type, no other arithmetic), clip_embed per element within the bound
built from its rounding points.  Samples and the window permutation come from the host plan entries (lr_vision_sample_plan,
lr_qwen_vision_plan), so the plan that runs in the product feeds the kernel that runs in the product.  Inputs are followed by poison
(NaN rows; index tables continue with indices of NaN rows, so that a read past a table shows in the result and stays inside the
allocation), outputs sit between sentinel guard rows, and every launch checks that nothing else was written.  Refusals are tested
through LR_EINVAL of calls that launch nothing.  The last test prints the largest clip_embed err / bound."""
import numpy as np
import pytest
import torch

from helpers import vision_ref as vr
from helpers.guards import DEV, Out, P, _in, _stream
from llava_reward_amd import _lib as L

pytestmark = pytest.mark.gpu

CODE = {"bf16": L.LR_DT_BF16, "f16": L.LR_DT_F16}
PIX = {"f32": L.LR_DT_F32, "bf16": L.LR_DT_BF16}
LR_EINVAL = 1                  # include/llava_reward_hip.h
NAN = float("nan")
RATIOS = {}                    # clip_embed case -> err / bound (printed by the last test)
I32 = torch.int32


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return L.load()


def _bits16(t):
    return t.contiguous().view(torch.int16)


def _vec(a, fill, dtype=I32, extra=16):
    """A flat array followed by `extra` elements of `fill`."""
    t = torch.as_tensor(np.asarray(a)).to(dtype).flatten()
    buf = torch.full((t.numel() + extra,), fill, dtype=dtype, device=DEV)
    buf[:t.numel()] = t.to(DEV)
    return buf


def _table(rows, poison_row, extra=4):
    """An int32 table [n, k] followed by `extra` rows holding poison_row (a record that points at NaN rows inside the allocation)."""
    t = torch.as_tensor(np.asarray(rows)).to(I32)
    buf = torch.tensor([list(poison_row)] * (t.shape[0] + extra), dtype=I32)
    buf[:t.shape[0]] = t
    return buf.to(DEV)


def _equal_bits(out, want, what):
    got = _bits16(out.body.cpu())
    want = _bits16(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(got, want), (what, int((got != want).sum()), "elements differ; first at", torch.nonzero(got != want)[0].tolist())


# ---------------------------------------------------------------------------------------------------------------------------------------
# im2col
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vr.im2col_cases(), ids=lambda c: "-".join(map(str, c)))
def test_im2col_bit_for_bit(lib, case):
    Pi = vr.make_im2col(case)
    nsrc = Pi.pix.shape[0]
    pix = _in(Pi.pix.reshape(nsrc, -1), fill=NAN, extra_rows=2)                      # crops nsrc, nsrc + 1: NaN
    crop_src = _vec(Pi.crop_src, nsrc)                                               # behind the table: the NaN crop
    rows = Pi.ncrop * Pi.g * Pi.g
    for dt in vr.DTS:
        for prec in (0, 1):
            out = Out(rows, Pi.Kpad << prec, dtype=vr.TDT[dt])
            rc = lib.lr_op_im2col(P(pix), PIX[Pi.pt], P(crop_src), Pi.ncrop, Pi.img, Pi.patch, Pi.Kpad, out.ptr, CODE[dt], prec, _stream())
            torch.cuda.synchronize()
            assert rc == 0, (case, dt, prec)
            out.check("im2col")
            _equal_bits(out, vr.im2col_ref(Pi, dt, prec), (case, dt, prec))
            pad = out.body[:, Pi.K:Pi.Kpad] if not prec else torch.cat([out.body[:, Pi.K:Pi.Kpad], out.body[:, Pi.Kpad + Pi.K:]], dim=1)
            assert bool((_bits16(pad) == 0).all()), "pad columns are +0 in hi and lo"


# ---------------------------------------------------------------------------------------------------------------------------------------
# clip_embed
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vr.clip_embed_cases(), ids=lambda c: f"H{c[0]}-T{c[1]}")
def test_clip_embed_within_bound(lib, case):
    Pc = vr.make_clip_embed(case)
    n, T, H = Pc.ncrop, Pc.T, Pc.H
    po, pos = _in(Pc.patch_out, fill=NAN), _in(Pc.pos, fill=NAN)
    cls, w, b = (_vec(t, NAN, dtype=torch.float32) for t in (Pc.cls, Pc.w, Pc.b))
    out = Out(n * T, H)
    assert (n * T) % 4 != 0
    rc = lib.lr_op_clip_embed(P(po), P(cls), P(pos), P(w), P(b), out.ptr, n, T, H, Pc.eps, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    out.check("clip_embed")
    got = out.body.cpu()
    y, e = vr.clip_embed_run(Pc, torch.float64)
    err = (got.double() - y).abs()
    r = vr.ratio(err, e)
    print(f"[clip_embed H{H} T{T}] max err/bound {r:.3g}  max err {float(err.max()):.3g}")
    assert r <= 1.0, (case, r)
    RATIOS[case] = r
    # row 0 of every crop reads cls (+ pos[0]): the same inputs, so the same bits
    for c in range(1, n):
        assert torch.equal(got[c * T].view(I32), got[0].view(I32)), f"row 0 of crop {c}"


# ---------------------------------------------------------------------------------------------------------------------------------------
# hd_gather
# ---------------------------------------------------------------------------------------------------------------------------------------
def _hd_launch(lib, clipx, samples, B, rows, g, H, sub_gn, glb_gn, dt, prec):
    """clipx [crops, T, H] (CPU): two NaN crops are put behind it, and the sample table continues with records that read them."""
    nc = clipx.shape[0]
    cx = _in(clipx.reshape(nc * (g * g + 1), H), fill=NAN, extra_rows=2 * (g * g + 1))
    smp = _table(samples, (1, 1, nc, 0))
    sub, glb = _vec(sub_gn, NAN, dtype=torch.float32), _vec(glb_gn, NAN, dtype=torch.float32)
    out = Out(rows, (4 * H) << prec, dtype=vr.TDT[dt])
    rc = lib.lr_op_hd_gather(P(cx), P(smp), B, rows, g * g + 1, H, P(sub), P(glb), out.ptr, CODE[dt], prec, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (g, H, B, dt, prec)
    out.check("hd_gather")
    return out


@pytest.mark.parametrize("case", vr.hd_gather_cases(), ids=lambda c: f"g{c[0]}-H{c[1]}-B{c[2]}")
def test_hd_gather_bit_for_bit(lib, case):
    Ph = vr.make_hd_gather(case)
    clipx = Ph.clipx.clone()
    clipx[~Ph.used] = NAN                                         # the gaps between the samples' crops
    for dt in vr.DTS:
        for prec in (0, 1):
            out = _hd_launch(lib, clipx, Ph.samples, Ph.B, Ph.rows, Ph.g, Ph.H, Ph.sub_gn, Ph.glb_gn, dt, prec)
            _equal_bits(out, vr.hd_gather_ref(Ph, dt, prec), (case, dt, prec))


# ---------------------------------------------------------------------------------------------------------------------------------------
# clip_tokens
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vr.clip_tokens_cases(), ids=lambda c: f"T{c[0]}-H{c[1]}-n{c[2]}")
def test_clip_tokens_bit_for_bit(lib, case):
    Pt = vr.make_clip_tokens(case)
    cx = _in(Pt.clipx, fill=NAN)
    rows = Pt.ncrop * (Pt.T - 1)
    for dt in vr.DTS:
        for prec in (0, 1):
            out = Out(rows, Pt.H << prec, dtype=vr.TDT[dt])
            rc = lib.lr_op_clip_tokens(P(cx), out.ptr, Pt.ncrop, Pt.T, Pt.H, CODE[dt], prec, _stream())
            torch.cuda.synchronize()
            assert rc == 0
            out.check("clip_tokens")
            _equal_bits(out, vr.clip_tokens_ref(Pt, dt, prec), (case, dt, prec))


# ---------------------------------------------------------------------------------------------------------------------------------------
# llava_pack
# ---------------------------------------------------------------------------------------------------------------------------------------
def _llava_launch(lib, proj, samples, g, D, rows, newline):
    """proj [crops, g g, D] (CPU): two NaN crops behind it, the sample table continues with records that read them."""
    nc = proj.shape[0]
    pj = _in(proj.reshape(nc * g * g, D), fill=NAN, extra_rows=2 * g * g)
    smp = _table(samples, (1, 1, 0, g, 0, g, nc, 0))
    nl = _vec(newline, NAN, dtype=torch.float32)
    out = Out(rows, D)
    rc = lib.lr_op_llava_pack(P(pj), P(smp), len(samples), rows, g, D, P(nl), out.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (g, D, len(samples))
    out.check("llava_pack")
    return out


def _plan_geoms(lib, sizes, crop, g):
    """The plan entry's (gh, gw, r0, r1, c0, c1) of every size; equal to the reference plan's."""
    pins = vr.pinpoints(crop)
    geoms = []
    for h, w in sizes:
        rc, smp, nc, nr = vr.lib_sample_plan(lib, vr.LR_BACKBONE_LLAVA_NEXT, crop, g, pins, h, w)
        assert rc == 0 and tuple(smp[:6]) + (nc, nr) == vr.llava_plan_ref(h, w, pins, crop, g), (h, w, smp)
        geoms.append(tuple(smp[:6]))
    return geoms


@pytest.mark.parametrize("case", vr.llava_pack_cases(), ids=lambda c: f"g{c[0]}-D{c[1]}-B{c[2]}")
def test_llava_pack_equal(lib, case):
    g, D, B = case
    Pl = vr.make_llava_pack(case, _plan_geoms(lib, vr.llava_pack_sizes(14 * g)[B], 14 * g, g))
    proj = Pl.proj.clone()
    used = torch.zeros(proj.shape[0], dtype=torch.bool)
    for gh, gw, _, _, _, _, crop0, _ in Pl.samples.tolist():
        used[crop0:crop0 + 1 + gh * gw] = True
    proj[~used] = NAN
    out = _llava_launch(lib, proj, Pl.samples, g, D, Pl.rows, Pl.newline)
    want = vr.llava_pack_ref(Pl.proj, Pl.samples, g, Pl.newline)
    assert want.shape == (Pl.rows, D)
    assert torch.equal(out.body.cpu().view(I32), want.view(I32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# qwen_patch_gather
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qwen_src(lib):
    rc, q = vr.lib_qwen_plan(lib, vr.QWEN_GATHER_GRID)
    assert rc == 0 and np.array_equal(q.src, vr.qwen_window_plan_ref(vr.QWEN_GATHER_GRID, vr.QWEN_MERGE, vr.QWEN_WS).src)
    return q.src


@pytest.mark.parametrize("case", vr.qwen_gather_cases(), ids=lambda c: "-".join(map(str, c)))
def test_qwen_patch_gather_bit_for_bit(lib, qwen_src, case):
    Pq = vr.make_qwen_gather(case, qwen_src)
    assert not np.array_equal(Pq.src, np.arange(Pq.rows)) and int(Pq.src.max()) < Pq.pix.shape[0]
    pix = _in(Pq.pix, fill=NAN)
    src = _vec(Pq.src, Pq.pix.shape[0])                           # behind the table: the first NaN row
    for dt in vr.DTS:
        for prec in (0, 1):
            out = Out(Pq.rows, Pq.Kpad << prec, dtype=vr.TDT[dt])
            rc = lib.lr_op_qwen_patch_gather(P(pix), PIX[Pq.pt], P(src), Pq.rows, Pq.K, Pq.Kpad, out.ptr, CODE[dt], prec, _stream())
            torch.cuda.synchronize()
            assert rc == 0
            out.check("qwen_patch_gather")
            _equal_bits(out, vr.qwen_gather_ref(Pq, dt, prec), (case, dt, prec))
            pad = out.body[:, Pq.K:Pq.Kpad] if not prec else torch.cat([out.body[:, Pq.K:Pq.Kpad], out.body[:, Pq.Kpad + Pq.K:]], dim=1)
            assert bool((_bits16(pad) == 0).all()), "pad columns are +0 in hi and lo"


# ---------------------------------------------------------------------------------------------------------------------------------------
# the plan entry's output drives the kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_hd_plan_feeds_hd_gather(lib):
    """Two images: lr_vision_sample_plan's records, laid end to end as run_vision lays them, go into the kernel; the result is the
    reference built from (h, w) alone."""
    g, H, crop = 4, 64, 56
    sizes = [(2 * crop, 3 * crop), (crop, 2 * crop)]
    smp, nc, rows = [], 0, 0
    for h, w in sizes:
        rc, s, ncr, nr = vr.lib_sample_plan(lib, vr.LR_BACKBONE_PHI3V, crop, g, None, h, w)
        assert rc == 0
        smp.append((s[0], s[1], nc, rows))
        nc += ncr
        rows += nr
    clipx = torch.randn(nc, g * g + 1, H, generator=torch.Generator().manual_seed(5))
    sub_gn, glb_gn = torch.randn(4 * H, generator=torch.Generator().manual_seed(6)), torch.randn(4 * H, generator=torch.Generator().manual_seed(7))
    ref_smp, _, ref_rows = vr.hd_layout([(h // crop, w // crop) for h, w in sizes], (0, 0), g)
    assert rows == ref_rows
    want = vr._encode(vr.hd_gather_values(clipx, ref_smp, g, sub_gn, glb_gn), "f16", 1)
    out = _hd_launch(lib, clipx, np.array(smp, np.int32), 2, rows, g, H, sub_gn, glb_gn, "f16", 1)
    _equal_bits(out, want, "plan -> hd_gather")


def test_llava_plan_feeds_llava_pack(lib):
    g, D, crop = 4, 64, 56
    sizes = [(70, 140), (200, 31)]
    pins = vr.pinpoints(crop)
    smp, nc, rows = [], 0, 0
    for h, w in sizes:
        rc, s, ncr, nr = vr.lib_sample_plan(lib, vr.LR_BACKBONE_LLAVA_NEXT, crop, g, pins, h, w)
        assert rc == 0
        smp.append(tuple(s[:6]) + (nc, rows))
        nc += ncr
        rows += nr
    proj = torch.randn(nc, g * g, D, generator=torch.Generator().manual_seed(8))
    newline = torch.randn(D, generator=torch.Generator().manual_seed(9))
    ref_smp, _, ref_rows = vr.llava_layout([vr.llava_plan_ref(h, w, pins, crop, g)[:6] for h, w in sizes], (0, 0), g)
    assert rows == ref_rows and {s[1] for s in ref_smp} == {2, 1}
    out = _llava_launch(lib, proj, np.array(smp, np.int32), g, D, rows, newline)
    assert torch.equal(out.body.cpu().view(I32), vr.llava_pack_ref(proj, ref_smp, g, newline).view(I32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals, report
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_vision_refusals_launch_nothing(lib):
    st = _stream()
    f32 = _in(torch.ones(64, 64))
    i32 = torch.zeros(64, dtype=I32, device=DEV)
    smp4 = _table([(1, 1, 0, 0)], (1, 1, 0, 0))
    smp8 = _table([(1, 1, 0, 2, 0, 2, 0, 0)], (1, 1, 0, 2, 0, 2, 0, 0))
    o16, o32 = Out(64, 64, dtype=torch.float16), Out(64, 64)
    F16, F32 = CODE["f16"], L.LR_DT_F32
    calls = [
        ("im2col patch 0", lambda: lib.lr_op_im2col(P(f32), F32, P(i32), 1, 6, 0, 16, o16.ptr, F16, 0, st)),
        ("im2col img % patch", lambda: lib.lr_op_im2col(P(f32), F32, P(i32), 1, 7, 2, 16, o16.ptr, F16, 0, st)),
        ("im2col Kpad < K", lambda: lib.lr_op_im2col(P(f32), F32, P(i32), 1, 6, 2, 8, o16.ptr, F16, 0, st)),
        ("im2col pixel type", lambda: lib.lr_op_im2col(P(f32), L.LR_DT_F16, P(i32), 1, 6, 2, 16, o16.ptr, F16, 0, st)),
        ("clip_embed H % 4", lambda: lib.lr_op_clip_embed(P(f32), P(f32), P(f32), P(f32), P(f32), o32.ptr, 1, 3, 6, 1e-5, st)),
        ("clip_embed H > 4096", lambda: lib.lr_op_clip_embed(P(f32), P(f32), P(f32), P(f32), P(f32), o32.ptr, 1, 3, 4100, 1e-5, st)),
        ("clip_embed T < 2", lambda: lib.lr_op_clip_embed(P(f32), P(f32), P(f32), P(f32), P(f32), o32.ptr, 1, 1, 8, 1e-5, st)),
        ("hd_gather H % 4", lambda: lib.lr_op_hd_gather(P(f32), P(smp4), 1, 5, 5, 6, P(f32), P(f32), o16.ptr, F16, 0, st)),
        ("hd_gather g odd", lambda: lib.lr_op_hd_gather(P(f32), P(smp4), 1, 5, 10, 4, P(f32), P(f32), o16.ptr, F16, 0, st)),
        ("hd_gather T not g g + 1", lambda: lib.lr_op_hd_gather(P(f32), P(smp4), 1, 5, 6, 4, P(f32), P(f32), o16.ptr, F16, 0, st)),
        ("hd_gather B 0", lambda: lib.lr_op_hd_gather(P(f32), P(smp4), 0, 5, 5, 4, P(f32), P(f32), o16.ptr, F16, 0, st)),
        ("clip_tokens H % 4", lambda: lib.lr_op_clip_tokens(P(f32), o16.ptr, 1, 3, 6, F16, 0, st)),
        ("clip_tokens T < 2", lambda: lib.lr_op_clip_tokens(P(f32), o16.ptr, 1, 1, 8, F16, 0, st)),
        ("llava_pack D % 4", lambda: lib.lr_op_llava_pack(P(f32), P(smp8), 1, 10, 2, 6, P(f32), o32.ptr, st)),
        ("llava_pack g 0", lambda: lib.lr_op_llava_pack(P(f32), P(smp8), 1, 10, 0, 8, P(f32), o32.ptr, st)),
        ("llava_pack B 0", lambda: lib.lr_op_llava_pack(P(f32), P(smp8), 0, 10, 2, 8, P(f32), o32.ptr, st)),
        ("qwen_patch_gather Kpad % 4", lambda: lib.lr_op_qwen_patch_gather(P(f32), F32, P(i32), 1, 12, 14, o16.ptr, F16, 0, st)),
        ("qwen_patch_gather Kpad < K", lambda: lib.lr_op_qwen_patch_gather(P(f32), F32, P(i32), 1, 12, 8, o16.ptr, F16, 0, st)),
        ("qwen_patch_gather pixel type", lambda: lib.lr_op_qwen_patch_gather(P(f32), L.LR_DT_F16, P(i32), 1, 12, 16, o16.ptr, F16, 0, st)),
    ]
    for what, call in calls:
        assert call() == LR_EINVAL, what
        torch.cuda.synchronize()
        assert o16.untouched() and o32.untouched(), what


def test_zz_report_largest_clip_embed_ratio():
    print("\nclip_embed max err / bound per case (RSQRT_ULP = %d):" % vr.RSQRT_ULP)
    for k in sorted(RATIOS):
        print(f"  H{k[0]:<5d} T{k[1]:<3d} {RATIOS[k]:.3g}")
    assert set(RATIOS) == set(vr.clip_embed_cases()) and all(v <= 1.0 for v in RATIOS.values())
    print(f"  largest {max(RATIOS.values()):.3g}")
