"""Times the event tail of the DSEC target loader at the training step's sizes (B = 2 samples of 500 000 events, 480 x 640, 1 and 5
time bins) both ways, and writes profiles/voxel_ordered_bench.txt:
  * the per-sample chain of the default path: event_prep -> events_to_voxel_grid (fp32 atomics) -> events_norm (double atomics)
    per sample, then a stack;
  * the batched ordered path pipeline.events_voxel_batch: one cat per field, cmdax5_event_prep_batch, cmdax5_voxel_ordered,
    cmdax5_events_norm_batch;
  * the voxel grid alone both ways, on uniformly spread events and with 2 % of a sample's events on one hot pixel (segments of
    ~10 000 contributions: the workgroup sort).
Launch counts are those of the entry points' sources; a torch cat / stack counts as one launch.  Each timing is the median of `--reps`
CUDA-event intervals over `--inner` back-to-back calls.  The ordered grid is also compared with the oracle's CPU result (bitwise) and
with itself from run to run; for the atomic grid the run-to-run comparison is reported.

    python tools/voxel_bench.py [--out profiles/voxel_ordered_bench.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cmda_amd import ops, pipeline as pl  # noqa: E402
from cmda_amd.datasets import DSECDataset  # noqa: E402
from oracle import uda as ouda  # noqa: E402
from tools.isr_aug_bench import timed  # noqa: E402

H, W, N, B = 480, 640, 500000, 2


def chain(events, rect, bins, clips):
    """DSECDataset._voxel per sample + stack: (1 + 2 + 5) launches per sample, one for the stack"""
    grids = []
    for (t, x, y, p), clip in zip(events, clips):
        tn, xr, yr, pol = pl.event_prep(t, x, y, p, rect, H, W)
        grids.append(ops.events_norm(ops.events_to_voxel_grid(tn, xr, yr, pol, bins, H, W), clip))
    return torch.stack(grids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'voxel_ordered_bench.txt'))
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--inner', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    ds = DSECDataset(synthetic_length=B, synthetic_events=N, device=dev)
    rect = ds.rectify_map
    events = [tuple(a.to(dev) for a in ds.raw(i)[1:5]) for i in range(B)]
    clips = [(N - 1) / 500000 * 1.5] * B
    offsets = [0, N, 2 * N]
    cat = [torch.cat([ev[k] for ev in events]) for k in range(4)]
    prepped = pl.event_prep_batch(*cat, offsets, rect, H, W)
    hot = [a.clone() for a in prepped]
    for b in range(B):   # every 50th event of a sample on one pixel
        hot[1][b * N:(b + 1) * N:50] = 301.37
        hot[2][b * N:(b + 1) * N:50] = 200.61
    lines = [f'Event voxel grid, B = {B} x {N} events, {H} x {W}, on {torch.cuda.get_device_name(0)}; median [min, max] us per call, '
             f'{args.reps} x {args.inner} calls',
             f'{"case":66s} {"launches":>8s} {"us":>30s}']

    def row(name, launches, t):
        lines.append(f'{name:66s} {launches:8d} {t[0]:12.1f} [{t[1]:8.1f}, {t[2]:8.1f}]')

    def atomic_grids(ev, bins):
        return torch.stack([ops.events_to_voxel_grid(*[a[b * N:(b + 1) * N] for a in ev], bins, H, W) for b in range(B)])

    for bins in (1, 5):
        lines.append(f'-- bins = {bins}')
        a = timed(lambda: chain(events, rect, bins, clips), args.reps, args.inner)
        o = timed(lambda: pl.events_voxel_batch(events, rect, bins, H, W, clips), args.reps, args.inner)
        row('per-sample chain: prep, atomic voxel grid, events_norm; stack', 8 * B + 1, a)
        row('batched ordered path: 4 cats, prep, ordered voxel grid, norm', 4 + 1 + 8 + 3, o)
        lines.append(f'  ratio ordered / chain: {o[0] / a[0]:.2f}x')
        for tag, ev in (('uniform events', prepped), ('2 % of the events on one pixel', hot)):
            va = timed(lambda: atomic_grids(ev, bins), args.reps, args.inner)
            vo = timed(lambda: ops.events_voxel_ordered_batch(*ev, offsets, bins, H, W), args.reps, args.inner)
            row(f'  voxel grid alone, {tag}: atomic x {B} + stack', 2 * B + 1, va)
            row(f'  voxel grid alone, {tag}: ordered, one call', 8, vo)
            lines.append(f'    ratio ordered / atomic: {vo[0] / va[0]:.2f}x')
            got = ops.events_voxel_ordered_batch(*ev, offsets, bins, H, W)
            again = ops.events_voxel_ordered_batch(*ev, offsets, bins, H, W)
            torch.use_deterministic_algorithms(True)    # keeps the oracle's put_(accumulate=True) a sequential sum at this size
            ref = torch.stack([ouda.events_to_voxel_grid(*[a[b * N:(b + 1) * N].cpu() for a in ev], W, H, bins) for b in range(B)])
            torch.use_deterministic_algorithms(False)
            at1, at2 = atomic_grids(ev, bins), atomic_grids(ev, bins)
            lines.append(f'    ordered == oracle (CPU, sequential) bitwise: {torch.equal(got.cpu(), ref)}; ordered run-to-run identical: '
                         f'{torch.equal(got, again)}; atomic run-to-run identical: {torch.equal(at1, at2)} '
                         f'(max |atomic - oracle| {float((at1.cpu() - ref).abs().max()):.2e})')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
