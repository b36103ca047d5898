#!/usr/bin/env python
"""N captions of one image: scoring.score_captions (image prefix computed once) against custom_forward on the same rows.

Full Phi-3.5-V shapes with synthetic weights in the default operand form, one image that the HD transform cuts into a 4x4 grid, N = 32
captions of the bench's caption length (128 tokens).  The two paths are ALTERNATED in one process after a warm-up and timed with HIP
events; the log gets both times, their ratio, the share of the prefix build and of the suffix pass, the cache size and whether the
rewards are bit-equal.  Nothing is asserted on time.

    python tools/shared_prefix_bench.py [--rounds 5] [--captions 32] [--out profiles/shared_prefix.log]
    python tools/shared_prefix_bench.py --suffix-only --rounds 3      # the suffix pass alone, for a kernel trace of it"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "llava-reward_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from llava_reward_amd import scoring, synth  # noqa: E402
from llava_reward_amd.model import RewardModel  # noqa: E402
from llava_reward_amd.preprocess import hd_transform_batch, merge_text_and_image_slots  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--captions", type=int, default=32)
    ap.add_argument("--caption-len", type=int, default=128)
    ap.add_argument("--dtype", default="f16x2f8")
    ap.add_argument("--tiny", action="store_true", help="tiny shapes (a smoke run of the tool itself)")
    ap.add_argument("--suffix-only", action="store_true", help="after one prefix build, run only forward_prefixed (for rocprofv3 --kernel-trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_prefix.log"))
    a = ap.parse_args()
    seed, N = 1234, a.captions
    tok = synth.StandInTokenizer()
    cfg = synth.tiny_config() if a.tiny else synth.full_config()
    image = synth.synth_image(seed, "shared_prefix_bench", 336 if a.tiny else 1344, 336 if a.tiny else 1344, True)
    crops = 1 if a.tiny else 16
    alphabet = "abcdefghijklmnopqrstuvwxyz ,."
    caps = ["".join(alphabet[synth.splitmix64_scalar(synth.tensor_seed(seed, f"cap.{i}") + j) % len(alphabet)] for j in range(a.caption_len))
            for i in range(N)]
    pix, sizes, ntok = hd_transform_batch([image], crops, "cuda")
    rows = []
    for cap in caps:
        msg = {"role": "user", "content": f"<|image_1|>\n{cap}"}
        prompt = tok.apply_chat_template([msg], tokenize=False, add_generation_prompt=True)[:-22] + tok.eos_token
        rows.append(merge_text_and_image_slots(tok, prompt, [ntok[0]])[0][0])
    S = max(len(r) for r in rows)
    n_prefix, n_shared = scoring.plan_shared_prefix(rows)
    pad = 0
    ids = torch.full((N, S), pad, dtype=torch.long)
    mask = torch.zeros((N, S), dtype=torch.long)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = r
        mask[i, :len(r)] = 1
    ids, mask = ids.cuda(), mask.cuda()
    pixN, sizesN = pix.expand(N, -1, -1, -1, -1).contiguous(), sizes.expand(N, -1).contiguous()
    m = RewardModel(cfg, synth_seed=seed, max_batch=N, max_seq=S, max_crops=crops + 1, operand_dtype=a.dtype, calibrate=False).to("cuda").eval()

    ordinary = lambda: m.custom_forward(ids, mask, pixN, sizesN)[0].float()
    shared = lambda: scoring.score_captions(m, tok, image, caps, num_crops=crops, batch_size=N, pad_token_id=pad)
    if a.suffix_only:
        state = m.build_prefix(rows[0][:n_prefix], pix, sizes, total_len=S)
        for _ in range(a.rounds):
            m.forward_prefixed(state, ids[:, n_shared:], mask[:, n_shared:])
        torch.cuda.synchronize()
        print(f"suffix only: {a.rounds} x forward_prefixed, B = {N}, T = {S - n_shared}, n_shared = {n_shared}")
        return
    ref, got = ordinary(), shared()                                  # warm-up: twins, workspace growth, code objects
    torch.cuda.synchronize()
    equal = bool(torch.equal(ref, got))
    t_ord, t_sh, t_build, t_suffix = [], [], [], []
    for _ in range(a.rounds):                                        # alternated: both see the same clocks and the same cache state
        t_ord.append(timed(ordinary)[0])
        t_sh.append(timed(shared)[0])
        tb, state = timed(lambda: m.build_prefix(rows[0][:n_prefix], pix, sizes, total_len=S))
        t_build.append(tb)
        t_suffix.append(timed(lambda: m.forward_prefixed(state, ids[:, n_shared:], mask[:, n_shared:]))[0])
    med = statistics.median
    lines = [
        f"shared image prefix, {'tiny' if a.tiny else 'full Phi-3.5-V'} shapes, synthetic weights, operand form {a.dtype} (default form, no probe), {torch.cuda.get_device_name(0)}",
        f"N = {N} captions of {a.caption_len} tokens, one image, {ntok[0]} image tokens; rows of {S} tokens; common prefix {n_prefix}, n_shared {n_shared}, "
        f"suffix rows T = {S - n_shared}",
        f"rounds = {a.rounds}, alternated in one process after one warm-up of each path, HIP events; median (min) in ms",
        f"custom_forward on the {N} right-padded rows      : {med(t_ord):9.2f} ({min(t_ord):.2f})",
        f"score_captions (HD transform + prefix + suffix) : {med(t_sh):9.2f} ({min(t_sh):.2f})",
        f"  build_prefix alone                            : {med(t_build):9.2f} ({min(t_build):.2f})",
        f"  forward_prefixed alone                        : {med(t_suffix):9.2f} ({min(t_suffix):.2f})",
        f"ratio custom_forward / score_captions           : {med(t_ord) / med(t_sh):9.2f}x   (algorithmic, by FLOP count: ~14x at N = 32)",
        f"decoder positions, ordinary / shared            : {N * S} / {n_shared + N * (S - n_shared)} = {N * S / (n_shared + N * (S - n_shared)):.1f}x for THESE rows (the stand-in tokenizer spells the end token in 13 tokens)",
        f"cache size                                      : {state.nbytes / 2 ** 20:9.1f} MiB",
        f"rewards torch.equal(score_captions, custom_forward): {equal}",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
