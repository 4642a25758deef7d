"""Times the fused BasicBlock tail of ConvertAvgFusion at the training step's sizes (512 x 512 input, the four MiT-B5 levels, 4 samples
per level as in the fused student pass: 2 passes of 2, groups = 2), bf16 and fp32 storage, and writes profiles/fusion_conv_bench.txt:
  * ops.resavg_fwd: 1 launch for the four levels (4 reads + 1 write of every map);
  * ops.resavg_bwd: the reducing and the applying launch (5 reads; 5 reads + 4 writes) with the workspace clear and the fold;
  * ConvertAvgFusion.fwd + .bwd, and AttentionAvgFusion.fwd + .bwd on the same features in the same run, for comparison.
Each timing is the median [min, max] of `--reps` device-event intervals over `--inner` back-to-back calls after a warm-up, the
callables of a group timed in turns; the kernels once as eager launches from Python and once as a replayed graph of the same calls
(device time without the host's launch rate).  Bytes are computed from the shapes; the floor is bytes / 6.3 TB/s (the achievable HBM
rate of an MI355X): derived, not measured.  GPU only: without one the tool fails, no CPU number is reported.

    python tools/fusion_conv_bench.py [--out profiles/fusion_conv_bench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import cmda_amd  # noqa: E402,F401
import cmda_amd.runtime as rt  # noqa: E402
from cmda_amd import fusion as fu  # noqa: E402
from cmda_amd import ops  # noqa: E402
from tools.isr_aug_bench import timed  # noqa: E402
from tools.split_targets_bench import graphed  # noqa: E402

DIMS, STRIDES, SIZE, B, GROUPS = [64, 128, 320, 512], [4, 8, 16, 32], 512, 4, 2
HBM = 6.3e12   # bytes / s achievable


def in_turns(fns, reps, inner):
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(ts, fns):
            t.append(timed(fn, 1, inner)[0])
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def tail_levels(dt, dev, gen):
    fwd, bwd = [], []
    for c, s in zip(DIMS, STRIDES):
        rows = B * (SIZE // s) ** 2
        mk = lambda: torch.randn(rows, c, generator=gen).to(dt).to(dev)
        brs = [dict(z=mk(), x=mk(), mean=(torch.randn(GROUPS, c, generator=gen) * 0.1).to(dev), rstd=(torch.rand(GROUPS, c, generator=gen) + 0.5).to(dev),
                    gamma=(torch.rand(c, generator=gen) + 0.5).to(dev), beta=(torch.randn(c, generator=gen) * 0.2).to(dev)) for _ in range(2)]
        out = torch.empty(rows, c, dtype=dt, device=dev)
        fwd.append(dict(image=brs[0], events=brs[1], out=out, M=rows // GROUPS, C=c))
        zeros = lambda: torch.zeros(c, device=dev)
        bwd.append(dict(image=dict(brs[0], dgamma=zeros(), dbeta=zeros()), events=dict(brs[1], dgamma=zeros(), dbeta=zeros()), dout=mk(),
                        M=rows // GROUPS, C=c))
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fusion_conv_bench.txt'))
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('fusion_conv_bench: needs an MI355X; no CPU number is reported')
    dev = torch.device('cuda:0')
    elems = sum(B * (SIZE // s) ** 2 * c for c, s in zip(DIMS, STRIDES))
    lines = [f'ConvertAvgFusion tail, {SIZE} x {SIZE}, {B} samples per level (groups = {GROUPS}), levels {DIMS}, on {torch.cuda.get_device_name(0)}; '
             f'median [min, max] us per call, {args.reps} x {args.inner} calls, the callables of a group timed in turns',
             f'{elems} elements per map; floor = bytes from the shapes / {HBM / 1e12:.1f} TB/s (derived, not measured)']
    for dt in (torch.bfloat16, torch.float32):
        rt.set_compute_dtype(dt)
        gen = torch.Generator().manual_seed(5)
        esz = 2 if dt == torch.bfloat16 else 4
        fwd_lv, bwd_lv = tail_levels(dt, dev, gen)
        fns = [lambda: ops.resavg_fwd(fwd_lv, GROUPS), lambda: ops.resavg_bwd(bwd_lv, GROUPS)]
        nbytes = [5 * elems * esz, 14 * elems * esz]
        names = ['ops.resavg_fwd (1 launch; 4 reads + 1 write)', 'ops.resavg_bwd (reduce + apply, clear + fold; 10 reads + 4 writes)']
        lines.append(f'== {str(dt).replace("torch.", "")} storage')
        lines.append(f'{"case":72s} {"MB":>7s} {"floor us":>9s} {"us":>30s} {"floor / measured":>17s}')
        for title, calls in (('-- eager launches from Python', fns), ('-- replayed graph of the same calls', None)):
            if calls is None:
                graphs = [graphed(fn) for fn in fns]
                calls = [g.replay for g, _ in graphs]
            lines.append(title)
            for name, nb, t in zip(names, nbytes, in_turns(calls, args.reps, args.inner)):
                floor = nb / HBM * 1e6
                lines.append(f'{name:72s} {nb / 1e6:7.1f} {floor:9.1f} {t[0]:12.1f} [{t[1]:8.1f}, {t[2]:8.1f}] {floor / t[0]:16.1%}')
        # the modules on the same features: forward + backward, eager (as the uncaptured step runs them)
        feats = lambda: [(torch.randn(B * (SIZE // s) ** 2, c, generator=gen).to(dt).to(dev), SIZE // s, SIZE // s) for c, s in zip(DIMS, STRIDES)]
        fi, fe, dy = feats(), feats(), [t for t, _, _ in feats()]
        caf, att = fu.ConvertAvgFusion().to(dev).train(), fu.AttentionAvgFusion().to(dev).train()

        def step(m, **kw):
            def run():
                outs, saved = m.fwd(fi, fe, B, **kw)
                with ops.backward_scope():
                    m.bwd(saved, dy, B)
                    ops.gemm_flush_deferred()
            return run
        ts = in_turns([step(caf, groups=GROUPS), step(att)], max(5, args.reps // 3), 5)
        lines.append('-- modules, fwd + bwd, eager')
        for name, t in zip(('ConvertAvgFusion (groups = 2)', 'AttentionAvgFusion'), ts):
            lines.append(f'{name:72s} {"":7s} {"":9s} {t[0]:12.1f} [{t[1]:8.1f}, {t[2]:8.1f}]')
    rt.set_compute_dtype(torch.float32)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
