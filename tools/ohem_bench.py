"""Times the OHEM pixel sampler at the training step's sizes (B = 2, logits 128 x 128 x 19 -> 512 x 512 labels) in both modes
(thresh = 0.7 and thresh = None, min_kept = 100000: the reference's defaults) next to the call it precedes, ops.ce_upsample_fwd on the
same logits and labels with a weight map, and writes profiles/ohem_bench.txt:
  * ops.ohem_weight: 4 launches and the clearing of its counters (cmdax7_ohem_weight);
  * ops.ce_upsample_fwd: 1 launch and the fill of its accumulator -- the yardstick.
Each timing is the median of `--reps` CUDA-event intervals over `--inner` back-to-back calls, the three callables timed in turns;
once as eager launches from Python (the host's launch rate is part of the figure) and once as a replayed graph of the same calls (what
the captured DACS iteration pays).  Before timing, the weights of both modes are compared with a float64 restatement of
OHEMPixelSampler.sample at this size (pixels that differ; the kernel's keys are fp32).

    python tools/ohem_bench.py [--out profiles/ohem_bench.txt]
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
from tools.isr_aug_bench import timed  # noqa: E402
from tools.split_targets_bench import graphed  # noqa: E402

B, H_LO, W_LO, H, W, NC, THRESH, MIN_KEPT = 2, 128, 128, 512, 512, 19, 0.7, 100000


def in_turns(fns, reps, inner):
    """median [min, max] us per call of the callables, timed in turns (the same neighbours for all)"""
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(ts, fns):
            t.append(timed(fn, 1, inner)[0])
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def restated_weight(lg, lab, thresh):
    """OHEMPixelSampler.sample in float64 on the CPU"""
    up = F.interpolate(lg.permute(0, 3, 1, 2).double(), size=(H, W), mode='bilinear', align_corners=False)
    valid = lab != 255
    safe = torch.where(valid, lab, torch.zeros_like(lab)).unsqueeze(1)
    if thresh is not None:
        key = up.softmax(1).gather(1, safe).squeeze(1)
        srt = key[valid].sort()[0]
        thr = max(srt[min(MIN_KEPT * B, srt.numel() - 1)].item(), thresh)
        return valid & (key < thr), thr
    key = -up.log_softmax(1).gather(1, safe).squeeze(1)
    srt = key[valid].sort(descending=True)[0]
    thr = srt[min(MIN_KEPT * B, srt.numel()) - 1].item()
    return valid & (key >= thr), thr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ohem_bench.txt'))
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--inner', type=int, default=50)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(5)
    lg_c = torch.randn(B, H_LO, W_LO, NC, generator=gen) * 3
    lab_c = torch.randint(0, NC, (B, H // 16, W // 16), generator=gen).repeat_interleave(16, 1).repeat_interleave(16, 2)
    likely = F.interpolate(lg_c.permute(0, 3, 1, 2), size=(H, W), mode='nearest').argmax(1)
    lab_c = torch.where(torch.rand(B, H, W, generator=gen) < 0.6, likely, lab_c)   # a net that is right on 60 % of the pixels
    lab_c[:, :24] = 255
    lab_c = lab_c.contiguous()
    lg, lab = lg_c.to(dev), lab_c.to(dev)

    lines = [f'OHEM pixel sampler, B = {B}, {H_LO} x {W_LO} x {NC} -> {H} x {W}, min_kept = {MIN_KEPT}, on {torch.cuda.get_device_name(0)}; '
             f'median [min, max] us per call, {args.reps} x {args.inner} calls, the callables timed in turns']
    for name, thresh in (('thresh 0.7', THRESH), ('thresh None', None)):
        wt, keys, thr = ops.ohem_weight(lg, lab, H, W, thresh, MIN_KEPT, debug=True)
        torch.cuda.synchronize()
        want, thr64 = restated_weight(lg_c, lab_c, thresh)
        lines.append(f'{name}: {int(wt.sum())} of {int((lab_c != 255).sum())} valid pixels selected, threshold {thr.item():.7g} (float64 restatement '
                     f'{thr64:.7g}); pixels that differ from the restatement: {int((wt.cpu() != want.float()).sum())} of {B * H * W}')
    weight = ops.ohem_weight(lg, lab, H, W, THRESH, MIN_KEPT)
    lines.append(f'{"case":62s} {"launches":>8s} {"us":>30s}')

    def row(label, launches, t):
        lines.append(f'{label:62s} {launches:>8s} {t[0]:12.1f} [{t[1]:8.1f}, {t[2]:8.1f}]')

    fns = [lambda: ops.ohem_weight(lg, lab, H, W, THRESH, MIN_KEPT), lambda: ops.ohem_weight(lg, lab, H, W, None, MIN_KEPT),
           lambda: ops.ce_upsample_fwd(lg, lab, weight, H, W)]
    names = [('ops.ohem_weight, thresh = 0.7', '4+1'), ('ops.ohem_weight, thresh = None', '4+1'), ('ops.ce_upsample_fwd (the yardstick)', '1+1')]
    for title, calls in (('-- eager launches from Python', fns), ('-- replayed graph of the same calls', None)):
        if calls is None:
            graphs = [graphed(fn) for fn in fns]
            calls = [g.replay for g, _ in graphs]
        ts = in_turns(calls, args.reps, args.inner)
        lines.append(title)
        for (label, launches), t in zip(names, ts):
            row(label, launches, t)
        lines.append(f'  ratio to the CE forward: thresh = 0.7 {ts[0][0] / ts[2][0]:.2f}x, thresh = None {ts[1][0] / ts[2][0]:.2f}x')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
