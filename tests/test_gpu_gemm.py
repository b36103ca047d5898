"""Every GEMM kernel form (csrc/gemm.hip, csrc/gemm8.hip, csrc/gemm8_narrow.hip: every (kernel, operand type, K-loop form, epilogue
instantiation, tile shape) cell the lr_op_* entry points reach, and every tile walk) against the fp64 reference and per-element
rounding bound of tests/helpers/gemm_ref.py, at the tile, M, N, K, stride and 4 GiB edges.  Operands sit in allocations whose gap
columns and rows past M / N are poisoned; C sits between sentinel guard rows with sentinel gap columns, and every launch checks that
nothing outside rows < M, columns < N was written.  On the `exact` family fp32 and un-activated operand outputs are compared bit for
bit.  Every case prints its cell and max err / bound."""
import ctypes as C
import os

import pytest
import torch

from helpers import gemm_ref as gr
from helpers.rowops_ref import lo8_scales_decode
from llava_reward_amd import _lib as L

pytestmark = pytest.mark.gpu

CODE = {"bf16": L.LR_DT_BF16, "f16": L.LR_DT_F16}
GR = 3                         # sentinel guard rows before row 0 and after row M - 1 of C; poisoned rows after the operands' last row
S16, S32, S8 = 0x5A5A, 0x5A5A5A5A, 0x5A
DEV = "cuda"
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
RATIOS = {}                    # K-loop form -> largest err / bound seen (printed by the last test)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return L.load()


def P(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _padded(x, rows, ld, fill):
    """x [r, c] inside a [rows, ld] allocation filled with `fill` (poison in the gap columns and in the rows past r)."""
    if x.dtype == torch.uint8:
        buf = torch.full((rows, ld), fill, dtype=torch.uint8, device=DEV)
    else:
        buf = torch.full((rows, ld), fill, dtype=x.dtype, device=DEV)
    buf[:x.shape[0], :x.shape[1]] = x.to(DEV)
    return buf


def _launch(lib, entry, Pb, bufs, M, N, K, k2, ld, tile, flags):
    """The lr_op_* call of one case; returns the code."""
    code = CODE[Pb.dt]
    st = _stream()
    if entry == "bt":
        return lib.lr_op_gemm_bt(P(bufs["A"]), P(bufs["W"]), bufs["Cptr"], P(bufs.get("bias")), M, N, K, ld[0], ld[1], ld[2], Pb.epi, Pb.act,
                                 code, tile, st)
    if entry == "split":
        return lib.lr_op_gemm_bt_split(P(bufs["A"]), P(bufs["W"]), bufs["Cptr"], P(bufs.get("bias")), M, N, K, Pb.epi, Pb.act, code, tile, st)
    if entry == "ext":
        return lib.lr_op_gemm_bt_ext(P(bufs["A"]), P(bufs["W"]), P(bufs["T"]), P(bufs["B"]), P(bufs.get("Blo")), bufs["Cptr"], P(bufs.get("bias")),
                                     M, N, K, k2, 0 if Pb.kform == "ext" else 1, Pb.epi, Pb.act, code, st)
    if entry == "rope":
        return lib.lr_op_gemm_rope(P(bufs["A"]), P(bufs["W"]), bufs["Cptr"], P(bufs.get("bias")), P(bufs["cs"]), M, N, K, Pb.rope_cols,
                                   Pb.rope_hd, code, tile, st)
    if entry == "fp8":
        return lib.lr_op_gemm_fp8(P(bufs["A"]), P(bufs["ascale"]), P(bufs["W"]), P(bufs["wscale"]), bufs["Cptr"], P(bufs.get("bias")), M, N, K,
                                  ld[2], Pb.epi, Pb.act, code, st)
    if entry == "mixed":
        return lib.lr_op_gemm_bt_mixed(P(bufs["A"]), P(bufs["W"]), P(bufs["W8"]), P(bufs["scratch"]), bufs["Cptr"], P(bufs.get("bias")), M, N, K,
                                       Pb.epi, Pb.act, code, flags, bufs["wexp"], st)
    raise ValueError(entry)


ENTRY_OF = {"16bit": "bt", "split": "split", "ext": "ext", "ext_split": "ext", "ext_split_blo": "ext", "e4m3": "mixed", "e4m3_third": "mixed",
            "w8a8": "fp8"}


def run(lib, kform, dt, M, N, K, *, family="normal", epi=gr.EPI_OUT_F32, act=0, bias=False, tile=-1, k2=0, lo8=False, pads=(0, 0, 0),
        rope=(0, 0), narrow=None, bandchunk=None, c_shift=0, seed=0, refuse=False, expect_walk=None, problem=None, chunk=4096, label=""):
    """One launch; returns max(err / bound).  pads = extra columns of (lda, ldw, ldc) where the entry point takes strides; narrow /
    bandchunk: LR_GEMM_NARROW / LR_GEMM_BANDCHUNK for this launch; c_shift: C starts that many elements into its row (plain kernel)."""
    entry = "rope" if epi == gr.EPI_ROPE_OP else ENTRY_OF[kform]
    env = {"LR_GEMM_NARROW": narrow, "LR_GEMM_BANDCHUNK": bandchunk}
    prev = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        aligned = c_shift == 0 and (N + pads[2]) % 8 == 0
        if refuse:
            cell = ("refused",)
            kernel = "product"
        else:
            cell = gr.cell(entry, dt, M, N, K, epi, bias, tile=tile, kform=kform, cus=CUS, narrow=-1 if narrow is None else narrow, aligned=aligned)
            kernel = "plain" if cell[0] == "plain" else "product"
        Pb = problem or gr.make_problem(kform, family, dt, M, N, K, epi=epi, act=act, bias=bias, k2=k2, lo8_out=lo8, rope_cols=rope[0],
                                        rope_hd=rope[1], seed=seed, kernel=kernel)
        tdt = gr.TDT[dt]
        strided = entry == "bt"
        pa, pw, pc = pads if strided else (0, 0, pads[2] if entry == "fp8" else 0)
        fill8 = 0x7E                                              # e4m3 448: the one-byte operands' poison
        bufs = {}
        Acols = Pb.A.shape[1]
        bufs["A"] = _padded(Pb.A, Pb.M + GR, Acols + pa, fill8 if kform == "w8a8" else gr.POISON)
        bufs["W"] = _padded(Pb.W, Pb.N + GR, Pb.W.shape[1] + pw, fill8 if kform == "w8a8" else gr.POISON)
        if Pb.bias is not None:
            bufs["bias"] = _padded(Pb.bias[None, :], 1, Pb.N + 8, gr.POISON).view(-1)
        if entry == "ext":
            bufs["T"] = _padded(Pb.T, Pb.M + GR, Pb.T.shape[1], gr.POISON)
            bufs["B"] = _padded(Pb.B, Pb.N + GR, Pb.B.shape[1], gr.POISON)
            if Pb.Blo is not None:
                bufs["Blo"] = _padded(Pb.Blo, Pb.N + GR, Pb.B.shape[1], gr.POISON)
        if entry == "rope":
            bufs["cs"] = Pb.cs.to(DEV)
        if entry == "fp8":
            bufs["ascale"], bufs["wscale"] = Pb.ascale.to(DEV), Pb.wscale.to(DEV)
        flags = 0
        if entry == "mixed":
            third = kform == "e4m3_third"
            flags = 3 | (8 if third else 0) | (32 if lo8 else 0)
            bufs["W8"] = _padded(Pb.Wlo, Pb.N + GR, Pb.K, 0.0) if third else torch.zeros(N + GR, Pb.K, dtype=tdt, device=DEV)
            nb = lib.lr_op_lo8_scratch_bytes(M, Pb.K)
            bufs["scratch"] = torch.full((nb + (lib.lr_op_lo8_scratch_bytes(M, Pb.nout) if lo8 else 0) + 256,), 127, dtype=torch.uint8, device=DEV)
            bufs["wexp"] = (C.c_int * 2)(0, 0)
        # C between sentinel guard rows, sentinel gap columns
        f32_out = epi in (gr.EPI_OUT_F32, gr.EPI_RESADD_F32)
        nout = Pb.nout
        width = nout if (f32_out or not Pb.split_out) else 2 * nout
        ldc = width + pc + c_shift
        es = 4 if f32_out else 2
        Call = torch.full((GR + M + GR, ldc), S32 if f32_out else S16, dtype=torch.int32 if f32_out else torch.int16, device=DEV)
        Cv = Call.view(torch.float32 if f32_out else tdt)
        if epi == gr.EPI_RESADD_F32 and not refuse:
            Cv[GR:GR + M, c_shift:c_shift + nout] = Pb.res.to(DEV)
        bufs["Cptr"] = C.c_void_p(Call.data_ptr() + (GR * ldc + c_shift) * es)
        bufs["Cview"] = Cv[GR:GR + M, c_shift:c_shift + width]
        rc = _launch(lib, entry, Pb, bufs, M, N, K, k2, (Acols + pa, Pb.W.shape[1] + pw, ldc), tile, flags)
        torch.cuda.synchronize()
        sent = S32 if f32_out else S16
        if refuse:
            assert rc != 0 and bool((Call == sent).all()), "a refused launch wrote C"
            return 0.0
        assert rc == 0, (rc, cell)
        # canaries
        for r0 in range(0, GR + M + GR, 32768):
            blk = Call[r0:r0 + 32768]
            rows = torch.arange(r0, r0 + blk.shape[0], device=DEV)
            inside = (rows >= GR) & (rows < GR + M)
            assert bool((blk[~inside] == sent).all()), "write into the guard rows of C"
            assert bool((blk[:, :c_shift] == sent).all()) and bool((blk[:, c_shift + width:] == sent).all()), "write into the gap columns of C"
        body = bufs["Cview"]
        if lo8:                                                   # the residual half: nout bytes + nout untouched bytes
            raw = Call[GR:GR + M, nout:2 * nout].contiguous().view(torch.uint8)
            assert bool((raw[:, nout:] == S8).all()), "write behind the one-byte residual half"
            lo8v = raw[:, :nout].contiguous().view(torch.float8_e4m3fn).double()
            s2 = bufs["scratch"][lib.lr_op_lo8_scratch_bytes(M, K):]
            nkb = nout // 128
            E = lo8_scales_decode(s2, M, nout).double()
            lo_val = (lo8v.view(M, nkb, 128) * torch.exp2(E - 127)[:, :, None]).view(M, nout)
        Pg = Pb.to(DEV)
        worst, maxerr, bits_ok = 0.0, 0.0, True
        bit_check = Pb.exact and not lo8 and (f32_out or (epi == gr.EPI_OUT_OP and act == 0))
        for r0 in range(0, M, chunk):
            sl = slice(r0, min(M, r0 + chunk))
            y, bnd = gr.reference(Pg, rows=sl)
            if f32_out or not Pb.split_out:
                got = body[sl, :nout].double()
            elif lo8:
                got = body[sl, :nout].double() + lo_val[sl]
            else:
                got = body[sl, :nout].double() + body[sl, nout:].double()
            err = (got - y).abs()
            rr = gr.max_ratio(err, bnd)
            if rr > worst and rr > 1.0:                           # where: for reducing a failing case
                ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), (err > 0).double() * 1e300)
                i = int(ratio.argmax())
                r_, c_ = r0 + i // nout, i % nout
                extra = f" hi {body[r_, c_].item()!r} lo8 {lo_val[r_, c_].item()!r} E {E[r_, c_ // 128].item()}" if lo8 else ""
                print(f"  worst element ({r_}, {c_}): got {got.flatten()[i].item()!r} want {y.flatten()[i].item()!r} bound {bnd.flatten()[i].item():.3g}{extra}")
            worst = max(worst, rr)
            maxerr = max(maxerr, err.max().item())
            if bit_check:
                want = gr.expected_bits(Pg, y)
                have = (body[sl, :nout],) if len(want) == 1 else (body[sl, :nout], body[sl, nout:])
                bits_ok = bits_ok and all(torch.equal(a, b) for a, b in zip(want, have))
        w = gr.walk(cell[0], M, N, cell[4], CUS, bandchunk=bandchunk != 0)
        print(f"[gemm {label} cell={cell} walk={w} M={M} N={N} K={K} k2={k2} {family} act={act} bias={bias} lo8={lo8} pads={pads}] "
              f"max err/bound {worst:.3g}  max err {maxerr:.3g}{'  bits equal' if bit_check and bits_ok else ''}")
        if expect_walk is not None:
            assert w == expect_walk, (w, expect_walk, CUS)
        assert bits_ok, ("exact family: output bits differ from the fp64 reference", cell, M, N, K)
        assert worst <= 1.0, (worst, cell, M, N, K, family)
        RATIOS[kform] = max(RATIOS.get(kform, 0.0), worst)
        return worst
    finally:
        for k, v in prev.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- every dispatch cell ----
def _fam(kform, n):
    fams = [f for f in gr.FAMILIES if not (f == "exact" and kform == "ext_split_blo")]
    return fams[n % len(fams)]


def _shape_for(epi, lo8, small_n=False):
    """(N, rope) with a partial last column tile: SwiGLU at N % 128 == 64, one-byte outputs at whole 128-column blocks, RoPE with the V
    part ending in an edge tile."""
    e = epi & 15
    if small_n:
        return (128 if lo8 else 120), (0, 0)
    if e == gr.EPI_SWIGLU_OP:
        return (768 if lo8 else 576), (0, 0)
    if e == gr.EPI_ROPE_OP:
        return 584, (512, 64)
    return (640 if lo8 else 520), (0, 0)


def _cell_cases():
    cases = []
    for n, c in enumerate(sorted(gr.all_cells())):
        kernel, dt, kform, epi, shape = c
        e = epi & 15
        tile = {(128, 128): 0, (256, 128): 1, (256, 256): 2}[shape] if kernel == "plain" else \
            {"deep_pf5": 3, "deep_pf5_persistent": 4, "deep_ab": 10, "product": 6}[kernel]
        narrow = None
        if kernel == "product" and dt == "f16" and kform != "w8a8":
            narrow = {(256, 256): 0, (128, 256): 1, (256, 128): None}[shape]
        small_n = shape == (256, 128) and kernel == "product"
        N, rope = _shape_for(epi, False, small_n)
        bias = bool(epi & 16) if e in (gr.EPI_SWIGLU_OP, gr.EPI_ROPE_OP) else (n % 2 == 0 and e != gr.EPI_RESADD_F32)
        K = 256 if kform in ("e4m3", "e4m3_third", "w8a8") else 192
        cases.append(dict(kform=kform, dt=dt, M=300, N=N, K=K, family=_fam(kform, n), epi=e, act=(n % 3 if e == gr.EPI_OUT_OP else 0), bias=bias,
                          tile=tile, k2=64 if kform.startswith("ext") else 0, rope=rope, narrow=narrow, seed=n))
    return cases


def _cell_of(c):
    entry = "rope" if c["epi"] == gr.EPI_ROPE_OP else ENTRY_OF[c["kform"]]
    return gr.cell(entry, c["dt"], c["M"], c["N"], c["K"], c["epi"], c["bias"], tile=c["tile"], kform=c["kform"], cus=CUS,
                   narrow=-1 if c["narrow"] is None else c["narrow"])


CELL_CASES = _cell_cases()
CELLS_HIT = {_cell_of(c) for c in CELL_CASES}
assert CELLS_HIT == gr.all_cells(), gr.all_cells() ^ CELLS_HIT          # the parametrisation reaches every cell, whatever the CU count


def _cid(c):
    return (f"{c['kform']}-{c['dt']}-{gr.EPI_NAME[c['epi']]}{'+b' if c['bias'] else ''}-a{c['act']}-t{c['tile']}-n{c['narrow']}-N{c['N']}")


def test_parametrisation_hits_every_dispatch_cell():
    assert CELLS_HIT == gr.all_cells() and len(CELL_CASES) == len(gr.all_cells())


@pytest.mark.parametrize("i", range(len(CELL_CASES)), ids=[_cid(c) for c in CELL_CASES])
def test_dispatch_cell(lib, i):
    run(lib, label="cell", **CELL_CASES[i])


# ---- one-byte residual output (flag 32): a run-time path of the operand-out and SwiGLU epilogues of the e4m3 forms ----
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("kform", ["e4m3", "e4m3_third"])
@pytest.mark.parametrize("epi,act,bias", [(gr.EPI_OUT_OP, 0, True), (gr.EPI_OUT_OP, 1, False), (gr.EPI_OUT_OP, 2, True), (gr.EPI_SWIGLU_OP, 0, False),
                                          (gr.EPI_SWIGLU_OP, 0, True)])
def test_one_byte_residual_output(lib, dt, kform, epi, act, bias):
    for narrow, fam in ((0, "normal"), (1 if dt == "f16" else 0, "scaled")):
        N, _ = _shape_for(epi, True)
        run(lib, kform, dt, 300, N, 384, family=fam, epi=epi, act=act, bias=bias, lo8=True, narrow=narrow if dt == "f16" else None, seed=act, label="lo8")
    if epi == gr.EPI_OUT_OP and dt == "f16":
        run(lib, kform, dt, 300, 128, 256, family="normal", epi=epi, act=act, bias=bias, lo8=True, seed=7, label="lo8 256x128")


# ---- tile position: interior, M edge, N edge and corner tiles in one launch, and one partial tile alone ----
EPI_ALL = [(gr.EPI_OUT_F32, 0, True), (gr.EPI_OUT_F32, 0, False), (gr.EPI_RESADD_F32, 0, True), (gr.EPI_RESADD_F32, 0, False), (gr.EPI_OUT_OP, 0, True),
           (gr.EPI_OUT_OP, 1, True), (gr.EPI_OUT_OP, 2, False), (gr.EPI_SWIGLU_OP, 0, False), (gr.EPI_SWIGLU_OP, 0, True)]
POS_FORMS = [("16bit", 6, 192, 0), ("16bit", 0, 192, 0), ("split", 6, 192, 0), ("split", 0, 192, 0), ("ext", 6, 192, 64), ("ext_split", 6, 192, 64),
             ("ext_split_blo", 6, 192, 128), ("e4m3", 6, 384, 0), ("e4m3_third", 6, 384, 0), ("w8a8", 6, 256, 0)]


@pytest.mark.parametrize("e", range(len(EPI_ALL)), ids=[f"{gr.EPI_NAME[x[0]]}-a{x[1]}{'+b' if x[2] else ''}" for x in EPI_ALL])
@pytest.mark.parametrize("f", range(len(POS_FORMS)), ids=[f"{x[0]}-t{x[1]}" for x in POS_FORMS])
def test_tile_position(lib, f, e):
    kform, tile, K, k2 = POS_FORMS[f]
    epi, act, bias = EPI_ALL[e]
    n = f * len(EPI_ALL) + e
    dt = "f16" if n % 2 else "bf16"
    sw = epi == gr.EPI_SWIGLU_OP
    for j, (M, N) in enumerate(((513, 576 if sw else 520), (100, 64 if sw else 72))):
        run(lib, kform, dt, M, N, K, family=_fam(kform, n + j), epi=epi, act=act, bias=bias, tile=tile, k2=k2, narrow=0 if dt == "f16" else None,
            seed=n, label="position")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("bias", [False, True])
def test_tile_position_rope(lib, dt, bias):
    """rope_cols a multiple of 256, the V part ends in an edge tile; M and N edges and the corner in one launch."""
    for tile, fam in ((6, "normal"), (-1, "exact"), (4, "outlier")):
        run(lib, "16bit", dt, 513, 584, 192, family=fam, epi=gr.EPI_ROPE_OP, bias=bias, tile=tile, rope=(512, 64), narrow=0 if dt == "f16" else None,
            seed=tile + 2, label="position")
    run(lib, "16bit", dt, 300, 776, 256, family="scaled", epi=gr.EPI_ROPE_OP, bias=bias, tile=-1, rope=(768, 96), seed=9, label="position")


# ---- M edges (what narrow_choice flips on, forced both ways and left to the launcher) ----
@pytest.mark.parametrize("M", [1, 2, 31, 33, 127, 128, 129, 255, 256, 257, 511, 513])
def test_m_edges(lib, M):
    for n, narrow in enumerate((0, 1, None)):
        kform = ("16bit", "e4m3", "split")[(M + n) % 3]
        epi, act, bias = EPI_ALL[(M + 2 * n) % len(EPI_ALL)]
        N = 576 if epi == gr.EPI_SWIGLU_OP else 520
        run(lib, kform, "f16", M, N, 256, family=_fam(kform, M + n), epi=epi, act=act, bias=bias, tile=6 if kform != "e4m3" else -1, narrow=narrow,
            seed=M, label="M edge")
    run(lib, "16bit", "bf16", M, 264, 128, family="exact", epi=gr.EPI_OUT_OP, bias=True, tile=0, seed=M, label="M edge")
    run(lib, "w8a8", "bf16", M, 264, 128, family="scaled", epi=gr.EPI_OUT_F32, bias=True, seed=M, label="M edge")


# ---- N edges ----
@pytest.mark.parametrize("N", [8, 64, 72, 120, 128, 136, 248, 256, 264, 504, 520, 1000, 1152])
def test_n_edges(lib, N):
    for n, tile in enumerate((6, 0, -1, 1, 2, 3, 10)):
        kform = "split" if (N // 8 + n) % 2 else "16bit"
        epi, act, bias = EPI_ALL[(N // 8 + n) % 7]
        run(lib, kform, "f16" if n % 2 else "bf16", 300, N, 128, family=_fam(kform, N + n), epi=epi, act=act, bias=bias, tile=tile, seed=N, label="N edge")
    run(lib, "e4m3", "f16", 300, N, 256, family="scaled", epi=gr.EPI_RESADD_F32, bias=True, seed=N, label="N edge")
    run(lib, "w8a8", "f16", 300, N, 256, family="exact", epi=gr.EPI_OUT_OP, bias=True, seed=N, label="N edge")


@pytest.mark.parametrize("N", [13, 250, 517])
@pytest.mark.parametrize("tile", [0, -1])
def test_n_not_a_multiple_of_8_and_unaligned_c_take_the_plain_kernel(lib, N, tile):
    for dt, epi, act, bias, fam in (("bf16", gr.EPI_OUT_F32, 0, True, "exact"), ("f16", gr.EPI_OUT_OP, 1, True, "outlier"),
                                    ("f16", gr.EPI_RESADD_F32, 0, False, "scaled")):
        run(lib, "16bit", dt, 200, N, 192, family=fam, epi=epi, act=act, bias=bias, tile=tile, pads=(0, 0, 3), seed=N, label="N % 8")
        if epi != gr.EPI_OUT_OP:          # ([hi | lo] outputs want N % 8 == 0 on every kernel: refused below)
            run(lib, "split", dt, 200, N, 192, family=fam, epi=epi, act=act, bias=bias, tile=tile, seed=N, label="N % 8")
        else:
            run(lib, "split", dt, 200, N, 192, epi=epi, act=act, bias=bias, tile=tile, refuse=True,
                problem=gr.make_problem("split", fam, dt, 200, N, 192, epi=epi, act=act, bias=bias, seed=N), label="split out N % 8")
    # N a multiple of 8 but C not 16-byte aligned: pick_tile's route to tile 0
    run(lib, "16bit", "f16", 200, 512, 192, family="exact", epi=gr.EPI_OUT_F32, bias=True, tile=tile, c_shift=1, pads=(0, 0, 7), seed=N, label="unaligned C")
    run(lib, "16bit", "bf16", 200, 512, 192, family="normal", epi=gr.EPI_OUT_OP, act=2, tile=tile, c_shift=3, pads=(0, 0, 5), seed=N, label="unaligned C")


# ---- K edges: K-tile counts around the ring's slots and prefetch depth, one-tile segments ----
@pytest.mark.parametrize("kform,K,k2", gr.FORM_K, ids=[f"{f}-K{K}-k{k2}" for f, K, k2 in gr.FORM_K])
def test_k_edges(lib, kform, K, k2):
    M, N = (300, 256) if K > 4096 else (300, 264)
    tiles = (3, 4, 5, 6, 10, 0) if kform in ("16bit", "split") else (6,)
    n = 0
    for tile in tiles:
        for fam in (["exact", "normal"] if kform != "ext_split_blo" else ["normal", "scaled"]):
            dt = "f16" if n % 2 else "bf16"
            run(lib, kform, dt, M, N, K, family=fam, epi=gr.EPI_OUT_F32, bias=True, tile=tile, k2=k2, narrow=(n % 2) if dt == "f16" else None,
                seed=K + n, label="K edge")
            n += 1
    run(lib, kform, "f16", M, N, K, family="outlier", epi=gr.EPI_OUT_OP, act=0, bias=True, tile=6 if kform in ("16bit", "split") else -1, k2=k2, seed=K, label="K edge")


def test_adapter_segment_of_one_k_tile_between_long_segments(lib):
    for kform in ("ext", "ext_split", "ext_split_blo"):
        for fam in (("exact", "scaled") if kform != "ext_split_blo" else ("normal", "scaled")):
            run(lib, kform, "f16", 700, 520, 1024, family=fam, epi=gr.EPI_OUT_F32, bias=True, k2=64, seed=3, label="adapter")
            run(lib, kform, "bf16", 700, 576, 1024, family=fam, epi=gr.EPI_SWIGLU_OP, k2=64, seed=4, label="adapter")


# ---- strides ----
@pytest.mark.parametrize("pads", [(8, 0, 0), (0, 8, 0), (0, 0, 8), (8, 16, 24)])
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 6, 10])
def test_strides(lib, pads, tile):
    for n, (epi, act, bias) in enumerate(EPI_ALL):
        dt = "f16" if n % 2 else "bf16"
        N = 576 if epi == gr.EPI_SWIGLU_OP else 520
        run(lib, "16bit", dt, 300, N, 192, family=_fam("16bit", n + tile), epi=epi, act=act, bias=bias, tile=tile, pads=pads, narrow=(n // 2 % 2) if dt == "f16" else None,
            seed=n, label="strides")
    if pads[2]:
        run(lib, "w8a8", "f16", 300, 520, 256, family="exact", epi=gr.EPI_OUT_F32, bias=True, pads=pads, seed=1, label="strides")
        run(lib, "w8a8", "bf16", 300, 520, 256, family="normal", epi=gr.EPI_OUT_OP, act=1, pads=pads, seed=2, label="strides")


# ---- walks: fewer tiles than CUs / a grid that is no multiple of 8; dynamic claims; band-aligned chunks ----
@pytest.mark.parametrize("family", ["exact", "scaled"])
def test_walks(lib, family):
    assert CUS == 256, "the shapes below are chosen for the MI355X's 256 CUs"
    run(lib, "16bit", "f16", 513, 520, 128, family=family, tile=6, narrow=0, expect_walk="static", label="walk: 9 tiles")
    run(lib, "16bit", "bf16", 2300, 7000, 128, family=family, tile=6, expect_walk="static", label="walk: 252 tiles")
    run(lib, "16bit", "bf16", 5000, 4096, 128, family=family, tile=6, expect_walk="static", label="walk: 320 tiles")
    run(lib, "16bit", "bf16", 8200, 8192, 128, family=family, tile=6, expect_walk="dynamic", label="walk")
    run(lib, "16bit", "f16", 16643, 4096, 128, family=family, epi=gr.EPI_OUT_OP, bias=True, tile=6, narrow=0, expect_walk="dynamic_bands", label="walk")
    run(lib, "16bit", "bf16", 16643, 4096, 128, family=family, tile=6, bandchunk=0, expect_walk="dynamic", label="walk")
    run(lib, "e4m3", "f16", 16643, 4096, 128, family=family, epi=gr.EPI_RESADD_F32, narrow=0, expect_walk="dynamic_bands", label="walk")
    run(lib, "16bit", "bf16", 5000, 4096, 128, family=family, tile=4, expect_walk="static", label="walk")
    run(lib, "16bit", "bf16", 1100, 1100 // 8 * 8, 128, family=family, tile=3, expect_walk="one_tile", label="walk")


def test_every_walk_is_reached():
    hit = {("plain", "one_tile"), ("deep_pf5", "one_tile")}
    for kernel, M, N, bc in (("product", 513, 520, True), ("product", 8200, 8192, True), ("product", 16643, 4096, True), ("deep_pf5_persistent", 5000, 4096, True),
                             ("deep_ab", 300, 520, True)):
        hit.add((kernel, gr.walk(kernel, M, N, (256, 256), 256, bandchunk=bc)))
    assert hit == gr.ALL_WALKS


# ---- byte offsets above 2^32 into A and into C ----
@pytest.mark.parametrize("tile", [-1, 0])
def test_byte_offsets_above_4_gib(lib, tile):
    M, N, K = 140000, 256, 128
    # the last rows of A lie beyond 4 GiB: lda = 16384 two-byte elements
    run(lib, "16bit", "f16", M, N, K, family="exact", epi=gr.EPI_OUT_OP, bias=True, tile=tile, pads=(16384 - K, 0, 0), chunk=16384, label="A > 4 GiB")
    torch.cuda.empty_cache()
    # the last rows of C lie beyond 4 GiB: ldc = 8192 floats
    run(lib, "16bit", "bf16", M, N, K, family="exact", epi=gr.EPI_OUT_F32, bias=True, tile=tile, pads=(0, 0, 8192 - N), chunk=16384, label="C > 4 GiB")
    torch.cuda.empty_cache()


# ---- refusals: host-side checks; non-zero return, C untouched ----
def test_refusals(lib):
    run(lib, "16bit", "f16", 100, 256, 100, tile=6, refuse=True, problem=gr.make_problem("16bit", "normal", "f16", 100, 256, 128), label="K % 64")
    run(lib, "16bit", "f16", 100, 256, 100, tile=0, refuse=True, problem=gr.make_problem("16bit", "normal", "f16", 100, 256, 128), label="K % 64")
    run(lib, "split", "f16", 100, 256, 96, tile=6, refuse=True, problem=gr.make_problem("split", "normal", "f16", 100, 256, 128), label="kw % 64")
    run(lib, "ext_split", "f16", 100, 256, 128, k2=32, refuse=True, problem=gr.make_problem("ext_split", "normal", "f16", 100, 256, 128, k2=64), label="k2 % 64")
    run(lib, "e4m3", "f16", 100, 256, 192, refuse=True, problem=gr.make_problem("e4m3", "normal", "f16", 100, 256, 256), label="mixed K % 128")
    run(lib, "16bit", "f16", 100, 512, 128, epi=gr.EPI_ROPE_OP, rope=(128, 64), tile=6, refuse=True,
        problem=gr.make_problem("16bit", "normal", "f16", 100, 512, 128, epi=gr.EPI_ROPE_OP, rope_cols=128, rope_hd=64), label="rope_cols % 256")
    run(lib, "16bit", "f16", 100, 12, 128, tile=6, refuse=True, problem=gr.make_problem("16bit", "normal", "f16", 100, 16, 128), label="N % 8 deep")
    run(lib, "w8a8", "f16", 100, 256, 100, refuse=True, problem=gr.make_problem("w8a8", "normal", "f16", 100, 256, 128), label="w8a8 K % 128")


def test_zz_report_largest_ratio_per_form():
    for k in sorted(RATIOS):
        print(f"[gemm summary] {k}: largest max err / bound over this run {RATIOS[k]:.3g}")
