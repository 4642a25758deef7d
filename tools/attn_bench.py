#!/usr/bin/env python3
"""Micro-benchmark of the wide-head attention core (head dim 128 ... 1024: the fusion modules' single-head Blocks) on the shapes the two
reference configs produce at 2 + 2 samples and at the 440 x 640 evaluation size: the chunked fused kernels (attention_wide.hip) against
the GEMM + softmax path (CMDA_ATTN_WIDE=2 against 0) in the same process on the same tensors, forward and forward + backward.
Usage (GPU box): python tools/attn_bench.py [--iters 200] [--repeat 3]   -- prints us per call; HIP-event timing after warm-up."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmda_amd.runtime as rt  # noqa: E402
from cmda_amd import nn as K  # noqa: E402
from cmda_amd import ops  # noqa: E402

SHAPES = [   # (set, B, N, Nk, hd, backward)
    ('avg', 2, 4096, 256, 128, True), ('avg', 2, 1024, 256, 320, True), ('avg', 2, 256, 256, 512, True),
    ('cat', 2, 16384, 256, 128, True), ('cat', 2, 4096, 256, 256, True), ('cat', 2, 1024, 256, 640, True), ('cat', 2, 256, 256, 1024, True),
    ('eval', 1, 4400, 260, 128, False), ('eval', 1, 1120, 280, 320, False), ('eval', 1, 280, 280, 512, False)]


def timeit(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200, help='launches per timed window (at least 200)')
    ap.add_argument('--repeat', type=int, default=3, help='timed windows per entry: the spread is printed next to the median')
    args = ap.parse_args()
    iters = max(200, args.iters)
    dev = torch.device('cuda:0')
    rt.set_compute_dtype(torch.bfloat16)
    print(f'{"set":5s} {"B":>2s} {"N":>6s} {"Nk":>4s} {"hd":>5s}  {"pass":8s} {"fused us":>18s} {"unfused us":>18s}  ratio')
    for name, B, N, Nk, hd, bwd in SHAPES:
        C, scale = hd, hd ** -0.5
        r = lambda *s: torch.randn(*s, device=dev).bfloat16()
        q, kv, do = r(B * N, C), r(B * Nk, 2 * C), r(B * N, C)

        def fwd():
            return K.attention_fwd(q, kv, B, N, Nk, 1, C, scale, need_grad=bwd)

        def fwd_bwd():
            _, P = K.attention_fwd(q, kv, B, N, Nk, 1, C, scale)
            K.attention_bwd(do, q, kv, P, B, N, Nk, 1, C, scale)

        for label, fn in (('fwd', fwd),) + ((('fwd+bwd', fwd_bwd),) if bwd else ()):
            res = {}
            for rep in range(args.repeat):       # fused and unfused windows alternate
                for mode in ('fused', 'unfused'):
                    os.environ['CMDA_ATTN_WIDE'] = '2' if mode == 'fused' else '0'   # 2: every head dim, whatever the dispatch table says
                    assert (fwd()[1] is None) == (mode == 'fused'), 'the A/B switch did not select the path'
                    res.setdefault(mode, []).append(timeit(fn, iters))
            med = {m: sorted(v)[len(v) // 2] for m, v in res.items()}
            fmt = lambda v: f'{sorted(v)[len(v) // 2]:8.1f} [{min(v):6.1f},{max(v):6.1f}]'
            print(f'{name:5s} {B:2d} {N:6d} {Nk:4d} {hd:5d}  {label:8s} {fmt(res["fused"]):>18s} {fmt(res["unfused"]):>18s}  {med["fused"] / med["unfused"]:5.2f}')
    os.environ.pop('CMDA_ATTN_WIDE', None)


if __name__ == '__main__':
    main()
