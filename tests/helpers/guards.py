"""The guard-row, gap-column and poison discipline of the single-kernel GPU tests (tests/test_gpu_rowops.py, tests/test_gpu_plan.py):
inputs sit at the head of allocations whose unused rows and columns hold poison, outputs between sentinel guard rows with sentinel gap
columns, and every launch checks that nothing else was written."""
import ctypes as C

import torch

from . import gemm_ref as gr

GR = 16                        # sentinel guard rows around every output, poisoned rows behind every input (16 rows keep 16-byte alignment)
S16, S32, S8 = 0x5A5A, 0x5A5A5A5A, 0x5A
DEV = "cuda"


def P(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _in(x, fill=gr.POISON, ld=None, extra_rows=GR):
    """x (rows x cols after flattening the leading dimensions) at the head of a [rows + extra_rows, ld] allocation full of `fill`."""
    if x.dim() == 1:
        x2 = x.reshape(1, -1)
    else:                                                       # (reshape(-1, 0) is ambiguous: a K = 0 operand has rows and no columns)
        x2 = x.reshape(x.numel() // x.shape[-1] if x.shape[-1] else x.shape[0], x.shape[-1])
    ld = ld or max(x2.shape[1], 1)
    buf = torch.full((x2.shape[0] + extra_rows, ld), fill, dtype=x.dtype, device=DEV)
    buf[:x2.shape[0], :x2.shape[1]] = x2.to(DEV)
    return buf


class Out:
    """[GR + rows + GR, ld] of sentinel words; .ptr = row GR, .body = the rows x cols the kernel may write."""

    def __init__(self, rows, cols, ld=None, dtype=torch.float32):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.f32 = dtype == torch.float32
        self.all = torch.full((GR + rows + GR, self.ld), S32 if self.f32 else S16, dtype=torch.int32 if self.f32 else torch.int16, device=DEV)
        self.view = self.all.view(dtype)
        self.ptr = C.c_void_p(self.all.data_ptr() + GR * self.ld * (4 if self.f32 else 2))
        assert self.ptr.value % 16 == 0
        self.body = self.view[GR:GR + rows, :cols]

    def check(self, what):
        sent = S32 if self.f32 else S16
        assert bool((self.all[:GR] == sent).all()) and bool((self.all[GR + self.rows:] == sent).all()), f"{what}: write into the guard rows"
        assert bool((self.all[:, self.cols:] == sent).all()), f"{what}: write into the gap columns"

    def untouched(self):
        return bool((self.all == (S32 if self.f32 else S16)).all())
