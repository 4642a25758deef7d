"""Times the feature-consistency loss (ops.feat_consis, include/cmda_hip_ext9.h) at the training step's sizes -- 2 samples at
512 x 512, the four MiT feature levels [32768, 64], [8192, 128], [2048, 320], [512, 512]: 4.06 M elements per operand -- in bf16 and
fp32, inside a replayed graph, and writes profiles/feat_consis_bench.txt:
  * fused       one launch, loss and gradient (what a DACS pass pays): reads a, b, grad, writes grad;
  * loss only   one launch (forward_train's forward): reads a, b;
  * grad only   one launch (forward_train's backward): reads a, b, grad, writes grad;
  * torch ops   the same arithmetic composed from torch ops, per level: mse_loss, the scaling and the sum of the four values, and
                grad += coef * (a - b).
Each figure is the median [min, max] over `--reps` replays of a graph holding `--inner` back-to-back calls, the callables timed in
turns in ONE process; GB/s = the bytes the launch has to move over that time; the share of the HBM floor = those bytes at the measured
streaming rate of the part (6.29 TB/s, MI355X float4 copy) over the time.  The operands of one call (24 to 65 MB) fit the 256 MB
last-level cache, as they do in the step, where the features have just been written: a share above 100 % says so.  Before timing, the
fused launch is compared with the torch composition (loss relative, gradient relative to its maximum).

    python tools/feat_consis_bench.py [--out profiles/feat_consis_bench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from cmda_amd import ops  # noqa: E402

LEVELS = [(2 * 128 * 128, 64), (2 * 64 * 64, 128), (2 * 32 * 32, 320), (2 * 16 * 16, 512)]
LAM = 0.25
HBM_BPS = 6.29e12


def graph_of(fn, inner):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = [fn() for _ in range(inner)]
    return g, keep


def replay_us(g, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'feat_consis_bench.txt'))
    ap.add_argument('--reps', type=int, default=31)
    ap.add_argument('--inner', type=int, default=50)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    n = sum(r * c for r, c in LEVELS)
    lines = [f'feature-consistency loss, levels {LEVELS} ({n} elements per operand), lambda {LAM}, on {torch.cuda.get_device_name(0)}; '
             f'median [min, max] us per call over {args.reps} replays of a graph of {args.inner} calls, the callables timed in turns']
    one = torch.ones(1, device=dev)
    for dt in (torch.bfloat16, torch.float32):
        gen = torch.Generator().manual_seed(5)
        A = [(torch.randn(r, c, generator=gen) + 0.5).to(dt).to(dev) for r, c in LEVELS]
        B = [torch.randn(r, c, generator=gen).to(dt).to(dev) for r, c in LEVELS]
        G = [torch.zeros(r, c, dtype=dt, device=dev) for r, c in LEVELS]
        coef = [LAM * 2.0 / (r * c) for r, c in LEVELS]

        def composed(grad=True, loss=True):
            out = None
            if loss:
                out = sum(LAM * F.mse_loss(a, b) for a, b in zip(A, B))
            if grad:
                for a, b, g, k in zip(A, B, G, coef):
                    g.add_(a - b, alpha=k)
            return out

        # agreement first
        loss, _ = ops.feat_consis(A, B, LAM, gscale=one, grads=G)
        got = [g.float().clone() for g in G]
        for g in G:
            g.zero_()
        ref = composed()
        torch.cuda.synchronize()
        gerr = max(((x - g.float()).abs().max() / g.float().abs().max()).item() for x, g in zip(got, G))
        lines.append(f'-- {str(dt).split(".")[1]}: fused loss {loss.item():.7g}, torch ops {float(ref):.7g} (rel {abs(loss.item() - float(ref)) / float(ref):.2e}); '
                     f'gradient vs torch ops, rel to its max {gerr:.2e}')
        for g in G:
            g.zero_()
        es = A[0].element_size()
        cases = [('fused (loss + gradient), 1 launch', lambda: ops.feat_consis(A, B, LAM, gscale=one, grads=G), 4 * n * es),
                 ('loss only, 1 launch', lambda: ops.feat_consis(A, B, LAM), 2 * n * es),
                 ('gradient only, 1 launch', lambda: ops.feat_consis(A, B, LAM, gscale=one, grads=G, want_loss=False), 4 * n * es),
                 ('torch ops, loss + gradient', lambda: composed(), 4 * n * es),
                 ('torch ops, loss only', lambda: composed(grad=False), 2 * n * es),
                 ('torch ops, gradient only', lambda: composed(loss=False), 4 * n * es)]
        graphs = [graph_of(fn, args.inner) for _, fn, _ in cases]
        ts = [[] for _ in cases]
        for _ in range(args.reps):
            for t, (g, _) in zip(ts, graphs):
                t.append(replay_us(g, args.inner))
        lines.append(f'{"case":40s} {"us":>28s} {"MB moved":>9s} {"GB/s":>8s} {"HBM floor us":>13s} {"floor / time":>13s}')
        for (name, _, nbytes), t in zip(cases, ts):
            med = statistics.median(t)
            floor = nbytes / HBM_BPS * 1e6
            lines.append(f'{name:40s} {med:10.1f} [{min(t):7.1f}, {max(t):7.1f}] {nbytes / 1e6:9.1f} {nbytes / med / 1e3:8.0f} {floor:13.1f} {floor / med:12.0%}')
        del graphs
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
