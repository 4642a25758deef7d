"""Times the split train type's targets at the training step's sizes (B = 2, teacher logits 128 x 128 x 19 -> 512 x 512 labels,
10 drawn classes) both ways, and writes profiles/split_targets_bench.txt:
  * the composed sequence: uda.DACS._mix_targets' four ops (pseudo_label -> pseudo_weight -> class_mix_label / class_mix against a
    freshly filled map of ones), once per stream: 8 launches, 2 fills, 2 memsets;
  * the pair ops.split_mix_targets (cmdax6_split_targets, cmdax6_split_weights): 2 launches, 1 memset.
Launch counts are those of the sources.  Each timing is the median of `--reps` CUDA-event intervals over `--inner` back-to-back
calls, the two ways alternating; once as eager launches from Python (the host's launch rate is part of the figure) and once as a
replayed graph of the same calls (what the captured DACS iteration pays).  The outputs of both ways are compared (bitwise) first.

    python tools/split_targets_bench.py [--out profiles/split_targets_bench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cmda_amd import ops  # noqa: E402
from tools.isr_aug_bench import timed  # noqa: E402

B, H_LO, W_LO, H, W, NC, K, THR, TOP, BOTTOM = 2, 128, 128, 512, 512, 19, 10, 0.968, 15, 120


def composed(lg0, lg1, lab, classes):
    out = []
    for lg in (lg0, lg1):
        pseudo, _, count = ops.pseudo_label(lg, H, W, THR, want_prob=False)
        pw = ops.pseudo_weight(count, B, H, W, TOP, BOTTOM)
        ones = torch.ones(B, H, W, dtype=torch.float32, device=lab.device)
        mixed = ops.class_mix_label(lab, pseudo, lab, classes)
        weight = ops.class_mix(ones.view(B, 1, H, W), pw.view(B, 1, H, W), lab, classes).view(B, H, W)
        out.append((pseudo, count, mixed, weight))
    return out


def pair(lg0, lg1, lab, classes):
    return ops.split_mix_targets(lg0, lg1, lab, classes, THR, TOP, BOTTOM)


def alternating(fa, fb, reps, inner):
    """median [min, max] us per call of two callables, timed in turns (the same neighbours for both)"""
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fa, 1, inner)[0])
        tb.append(timed(fb, 1, inner)[0])
    return [(statistics.median(t), min(t), max(t)) for t in (ta, tb)]


def graphed(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    return g, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'split_targets_bench.txt'))
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--inner', type=int, default=50)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(5)
    lg0 = (torch.randn(B, H_LO, W_LO, NC, generator=gen) * 8).to(dev)
    lg1 = (torch.randn(B, H_LO, W_LO, NC, generator=gen) * 16).to(dev)
    lab = torch.randint(0, NC, (B, H // 16, W // 16), generator=gen).repeat_interleave(16, 1).repeat_interleave(16, 2)
    lab[:, :24] = 255
    lab = lab.contiguous().to(dev)
    classes = torch.full((B, K), -1, dtype=torch.int64)
    for b in range(B):
        classes[b] = torch.tensor([255] + torch.randperm(NC, generator=gen)[:K - 1].tolist())
    classes = classes.to(dev)

    ref, got = composed(lg0, lg1, lab, classes), pair(lg0, lg1, lab, classes)
    torch.cuda.synchronize()
    same = all(torch.equal(got[0][s], ref[s][0]) and int(got[1][s]) == int(ref[s][1]) and torch.equal(got[2][s], ref[s][2]) and
               torch.equal(got[3][s], ref[s][3]) for s in range(2))
    counts = [int(c) for c in got[1]]
    lines = [f'Split train type targets, B = {B}, {H_LO} x {W_LO} x {NC} -> {H} x {W}, K = {K}, on {torch.cuda.get_device_name(0)}; '
             f'median [min, max] us per call, {args.reps} x {args.inner} calls, the two ways alternating',
             f'pair == composed sequence, bitwise (pseudo-labels, counts, mixed labels, mixed weights): {same}; confident pixels {counts} of {B * H * W}',
             f'{"case":62s} {"launches":>8s} {"us":>30s}']

    def row(name, launches, t):
        lines.append(f'{name:62s} {launches:>8s} {t[0]:12.1f} [{t[1]:8.1f}, {t[2]:8.1f}]')

    fa, fb = (lambda: composed(lg0, lg1, lab, classes)), (lambda: pair(lg0, lg1, lab, classes))
    ea, eb = alternating(fa, fb, args.reps, args.inner)
    lines.append('-- eager launches from Python')
    row('composed: _mix_targets\' four ops, per stream', '8+2+2', ea)
    row('pair: ops.split_mix_targets', '2+1', eb)
    lines.append(f'  ratio pair / composed: {eb[0] / ea[0]:.2f}x')
    ga, _ka = graphed(fa)
    gb, _kb = graphed(fb)
    ra, rb = alternating(ga.replay, gb.replay, args.reps, args.inner)
    lines.append('-- replayed graph of the same calls')
    row('composed: _mix_targets\' four ops, per stream', '8+2+2', ra)
    row('pair: ops.split_mix_targets', '2+1', rb)
    lines.append(f'  ratio pair / composed: {rb[0] / ra[0]:.2f}x')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
