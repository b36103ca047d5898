"""Where the scaled 16x16x128 e4m3 MFMA (v_mfma_scale_f32_16x16x128_f8f6f4) loses bits, measured through lr_op_gemm_fp8 with unit scales:
one large product at k = 0 and one small product 225 x 2^q at k = row index, K = 128.  Prints, per exponent gap, the fraction of the
small product that reaches the fp32 result and the rows (= K positions) that share it.  On an MI355X: K positions 1 .. 7 (the large
product's group of 8) keep 224 / 225 at gaps 8 .. 12, 192 / 225 at 13, 128 / 225 at 14 and nothing from 15 on -- truncation towards zero
below 2^-13 of the group's largest product -- while every other position is exact down to the final fp32 rounding; a product of the
next K-tile against a 2^16 accumulator rounds as fp32 does.  tests/helpers/gemm_ref.py charges this as E_dot8.
Usage: python tools/e4m3_dot8_probe.py"""
import ctypes as C, sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "llava-reward_amd"), ROOT]
import torch
from llava_reward_amd import _lib as L
lib = L.load()
P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
M = N = K = 128
def launch(a, w):
    a8, w8 = a.to(torch.float8_e4m3fn), w.to(torch.float8_e4m3fn)
    assert torch.equal(a8.float(), a) and torch.equal(w8.float(), w)
    one = torch.ones(128, device="cuda")
    out = torch.zeros(M, N, device="cuda")
    assert lib.lr_op_gemm_fp8(P(a8.view(torch.uint8)), P(one), P(w8.view(torch.uint8)), P(one), P(out), None, M, N, K, N, L.EPI_OUT_F32, 0, L.LR_DT_F16, st) == 0
    torch.cuda.synchronize()
    return out.double()
for bigexp in (8, 4):
    big = 2.0 ** bigexp
    for q in range(8, -13, -1):
        x = -(-q // 2); y = q - x
        a = torch.zeros(M, K, device="cuda"); w = torch.zeros(N, K, device="cuda")
        a[:, 0] = big; w[:, 0] = big
        w[:, 1:] = 1.875 * 2.0 ** y
        idx = torch.arange(1, M, device="cuda")
        a[idx, idx] = 1.875 * 2.0 ** x
        v = 3.515625 * 2.0 ** q
        out = launch(a, w)
        kept = ((out[1:, 0] - big * big) / v)            # row m: small product at k = m
        vals = {}
        for m, r in enumerate(kept.tolist(), start=1):
            vals.setdefault(round(r, 6), []).append(m)
        gap = 2 * bigexp - q
        desc = "; ".join(f"{r}: {len(ms)} rows" + (f" {ms}" if len(ms) <= 16 else "") for r, ms in sorted(vals.items()))
        print(f"big 2^{2*bigexp} small 3.515625*2^{q} (gap {gap}): kept fraction -> {desc}", flush=True)
# accumulator input: C is zero in the kernel's first step; second K-tile adds to a large accumulator
K2 = 256
a = torch.zeros(M, K2, device="cuda"); w = torch.zeros(N, K2, device="cuda")
a[:, 0] = 256.0; w[:, 0] = 256.0
for q in (0, -4, -6, -8, -10, -12):
    x = -(-q // 2); y = q - x
    a[:, 128:] = 0; w[:, 128:] = 0
    a[:, 128] = 1.875 * 2.0 ** x; w[:, 128] = 1.875 * 2.0 ** y
    a8, w8 = a.to(torch.float8_e4m3fn), w.to(torch.float8_e4m3fn)
    one = torch.ones(128, device="cuda"); out = torch.zeros(M, N, device="cuda")
    assert lib.lr_op_gemm_fp8(P(a8.view(torch.uint8)), P(one), P(w8.view(torch.uint8)), P(one), P(out), None, M, N, K2, N, L.EPI_OUT_F32, 0, L.LR_DT_F16, st) == 0
    torch.cuda.synchronize()
    v = 3.515625 * 2.0 ** q
    print(f"accumulator 2^16 + next step's single product {v}: got - 2^16 = {out[0,0].item() - 65536.0} (fp32 nearest {float(torch.tensor(65536.0 + v, dtype=torch.float32)) - 65536.0})")
