"""The shared-key-prefix attention form (csrc/attention_shared.hip, lr_op_attention_shared) against the full launch it stands for.

Each case builds random Q / K / V of [B, S = n_shared + T], copies the first n_shared K / V rows of sequence 0 into every sequence and
runs the existing op on the whole thing; then the new entry runs on the own rows [B, T] alone, with those n_shared rows as the shared
image.  The own rows must come back BIT-EQUAL: the form is the full launch with the repeated work left out, not an approximation of it.
(n_shared, T) walk the dispatch bands of the total key count -- the instantiation is chosen on n_shared + T -- and the tile geometry:
a straddling query tile, own rows in two query tiles, a single own row.  Own-row masks have a different valid length per sequence.
One single and one split case are also held to the fp64 reference and per-element bound of tests/helpers/attention_ref.py."""
import ctypes as C

import pytest
import torch

from helpers import attention_ref as ar
from llava_reward_amd import _lib as L

pytestmark = pytest.mark.gpu

DT = {"bf16": (L.LR_DT_BF16, torch.bfloat16), "f16": (L.LR_DT_F16, torch.float16)}
GUARD = 3                      # canary rows in front of and behind O
SENTINEL = 0x5A5A
B = 3
# (n_shared, T): split<=128 | below 1024 (own rows in two 128-query tiles, one straddling) | ping-pong at 1024 + 37 and straddling 1024
# from below (960 + 130: the end-aligned shift applies) | one own row
SHAPES = [(64, 37), (256, 130), (1024, 37), (960, 130), (256, 1)]
FORMS = [(96, 4, 1), (128, 4, 4)]          # head_dim, heads, kv_group


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return L.load()


def P(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _case(dt, hd, H, group, split, NS, T, seed):
    """Packed [q | k | v] (| residuals) rows of the full problem and of its own / shared parts, on the device."""
    code, tdt = DT[dt]
    S, Hkv = NS + T, H // group
    valid = [T, max(1, T // 2), 1]                            # own-row masks: right padding of different lengths
    mask = torch.zeros(B, S, dtype=torch.int64)
    mask[:, :NS] = 1
    for b in range(B):
        mask[b, NS:NS + valid[b]] = 1
    q, k, v = ar.make_inputs("normal", B, S, H, Hkv, hd, scale=hd ** -0.5, mask=mask, seed=seed)
    k[:, :NS] = k[0, :NS]
    v[:, :NS] = v[0, :NS]
    wq, wkv = H * hd, Hkv * hd
    W = wq + 2 * wkv
    ld = 2 * W if split else W
    xs = [q.reshape(B * S, wq), k.reshape(B * S, wkv), v.reshape(B * S, wkv)]
    parts = [ar.split(x, tdt) if split else (x.to(tdt), None) for x in xs]
    rows = torch.zeros(B * S, ld, dtype=tdt)
    for off, (hi, lo) in zip((0, wq, wq + wkv), parts):
        rows[:, off:off + hi.shape[1]] = hi
        if split:
            rows[:, W + off:W + off + lo.shape[1]] = lo
    full = rows.cuda()
    r3 = full.view(B, S, ld)
    own = r3[:, NS:].contiguous().view(B * T, ld)
    shared = r3[0, :NS].contiguous()
    return dict(code=code, tdt=tdt, S=S, Hkv=Hkv, wq=wq, wkv=wkv, W=W, ld=ld, mask=mask.cuda(), full=full, own=own, shared=shared,
                parts=parts, scale=hd ** -0.5)


def _run_full(lib, c, hd, H, group, split, lazy):
    ldo = 2 * c["wq"] if split else c["wq"]
    O = torch.full((B * c["S"] + GUARD, ldo), SENTINEL, dtype=torch.int16, device="cuda").view(c["tdt"])
    kmin = torch.zeros(B, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    X = c["full"]
    offs = (0, c["wq"], c["wq"] + c["wkv"])
    if split:
        rc = lib.lr_op_attention_split_ex(P(X), P(X), P(X), P(O), P(c["mask"]), P(kmin), c["ld"], ldo, *offs, c["W"], c["wq"], B, c["S"], H, hd,
                                          1, group, c["scale"], lazy, c["code"], st)
    else:
        rc = lib.lr_op_attention(P(X), P(X), P(X), P(O), P(c["mask"]), P(kmin), c["ld"], ldo, *offs, B, c["S"], H, hd, 1, group, c["scale"],
                                 c["code"], st)
    torch.cuda.synchronize()
    assert rc == 0, lib.lr_last_error(None)
    return O[:B * c["S"]]


def _run_shared(lib, c, hd, H, group, split, lazy, NS, T):
    ldo = 2 * c["wq"] if split else c["wq"]
    O = torch.full((GUARD + B * T + GUARD, ldo), SENTINEL, dtype=torch.int16, device="cuda").view(c["tdt"])
    own_mask = c["mask"][:, NS:].contiguous()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    X, Sh = c["own"], c["shared"]
    offs = (0, c["wq"], c["wq"] + c["wkv"])
    rc = lib.lr_op_attention_shared(P(X), P(X), P(X), P(Sh), P(Sh), P(O[GUARD:]), P(own_mask), NS, c["ld"], ldo, *offs,
                                    c["W"] if split else 0, c["wq"] if split else 0, B, T, H, hd, group, c["scale"], lazy, c["code"], st)
    torch.cuda.synchronize()
    assert rc == 0, lib.lr_last_error(None)
    bits = O.view(torch.int16)
    assert bool((bits[:GUARD] == SENTINEL).all()), "write in front of the first own row"
    assert bool((bits[GUARD + B * T:] == SENTINEL).all()), "write past the last own row"
    return O[GUARD:GUARD + B * T]


CASES = [(hd, H, g, split, lazy) for hd, H, g in FORMS for split, lazy in ((False, 0.0), (True, 0.0), (True, 8.0))]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}+{s[1]}")
@pytest.mark.parametrize("form", CASES, ids=lambda f: f"hd{f[0]}-g{f[2]}-{'x2' if f[3] else 'x1'}-lazy{int(f[4])}")
def test_own_rows_bit_equal_to_the_full_launch(lib, dt, shape, form):
    hd, H, group, split, lazy = form
    NS, T = shape
    c = _case(dt, hd, H, group, split, NS, T, seed=NS + T + hd)
    full = _run_full(lib, c, hd, H, group, split, lazy)
    got = _run_shared(lib, c, hd, H, group, split, lazy, NS, T)
    want = full.view(B, c["S"], -1)[:, NS:].reshape(B * T, -1)
    assert bool(torch.isfinite(got.float()).all())
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
        f"{int((got.view(torch.int16) != want.view(torch.int16)).sum())} of {got.numel()} elements differ"


@pytest.mark.parametrize("split", [False, True], ids=["x1", "x2"])
def test_against_the_fp64_reference(lib, split):
    """The own rows against attention_ref.reference on the full problem, with that helper's own per-element bound."""
    dt, hd, H, group, lazy = "f16", 96, 4, 1, 8.0 if split else 0.0
    NS, T = 256, 130
    c = _case(dt, hd, H, group, split, NS, T, seed=5)
    got = _run_shared(lib, c, hd, H, group, split, lazy, NS, T)
    S, wq, Hkv = c["S"], c["wq"], c["Hkv"]
    val = got[:, :wq].double() + (got[:, wq:2 * wq].double() if split else 0)
    vals = [(hi.double() + lo.double()) if split else hi.double() for hi, lo in c["parts"]]
    shp = [(B, S, H, hd), (B, S, Hkv, hd), (B, S, Hkv, hd)]
    qd, kd, vd = (x.cuda().view(s) for x, s in zip(vals, shp))
    lo3 = [lo.double().cuda().view(s) for (_, lo), s in zip(c["parts"], shp)] if split else None
    ref, bnd = ar.reference(qd, kd, vd, scale=c["scale"], causal=True, mask=c["mask"], kv_group=group, dtype=dt, split=split, lo=lo3,
                            lazy_t=lazy, chunk=512)
    err = (val.view(B, T, H, hd) - ref[:, NS:]).abs()
    r = ar.max_ratio(err, bnd[:, NS:])
    print(f"[attn shared {dt}{'x2' if split else ''} hd={hd} n_shared={NS} T={T}] max err/bound {r:.3g}  max err {err.max().item():.3g}")
    assert r <= 1.0, r


def test_refusals(lib):
    """n_shared off the key tile, a missing shared image and a head_dim without the form are refused before anything is launched."""
    c = _case("f16", 96, 4, 1, False, 64, 8, seed=1)
    O = torch.full((B * 8, c["wq"]), SENTINEL, dtype=torch.int16, device="cuda").view(c["tdt"])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    X, Sh, m = c["own"], c["shared"], c["mask"][:, 64:].contiguous()
    offs = (0, c["wq"], c["wq"] + c["wkv"])
    for ns, sh, hd in ((60, Sh, 96), (64, None, 96), (64, Sh, 64)):
        rc = lib.lr_op_attention_shared(P(X), P(X), P(X), P(sh), P(sh), P(O), P(m), ns, c["ld"], c["wq"], *offs, 0, 0, B, 8, 4, hd, 1,
                                        c["scale"], 0.0, c["code"], st)
        torch.cuda.synchronize()
        assert rc != 0 and bool((O.view(torch.int16) == SENTINEL).all())
