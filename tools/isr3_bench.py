"""Times the multi-parameter ISR and the cow mask (ops.isr_multi, ops.cow_mask) against what the tree offered before them, and writes
profiles/isr3_bench.txt:
  * isr_multi [2,512,512], C = 3 against three ops.isr_from_gray calls, a channel pick and a cat;
  * isr_multi [2,540,960] with a 512 x 512 window per sample against the per-sample loop of DarkZurichICDataset's one-channel path
    (isr_from_gray of one frame, slice, flip, contiguous; cat), three times for the three parameter rows, then pick and cat;
  * cow_mask [2,3,512,512], K = 195 against the bytes it must move (the ISR read and written once).
Launch counts are those of the entry points' sources (kernel launches per call); torch's slice / flip / contiguous / cat copies are
counted as one launch each.  Each timing is the median of `--reps` CUDA-event intervals over `--inner` back-to-back calls.

    python tools/isr3_bench.py [--out profiles/isr3_bench.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cmda_amd import ops  # noqa: E402
from cmda_amd.datasets import ISR3_PRESETS  # noqa: E402
from tools.isr_aug_bench import timed  # noqa: E402

PRESET = ISR3_PRESETS['night']
VR = PRESET[0]['val_range']


def three_calls(gray):
    """the composition available without isr_multi: 3 x (init + minmax + apply, three identical planes each), pick, cat"""
    return torch.cat([ops.isr_from_gray(gray, VR, p['_threshold'], p['_clip_range'], p['shift_pixel'], 'rightdown')[:, :1] for p in PRESET], 1)


def loader_loop(gray, wins, ch, cw):
    """DarkZurichICDataset's one-channel path per parameter row: per sample the ISR of the whole frame, slice, flip, contiguous"""
    chans = []
    for p in PRESET:
        isr = []
        for b, (x, y, f) in enumerate(wins):
            v = ops.isr_from_gray(gray[b:b + 1], VR, p['_threshold'], p['_clip_range'], p['shift_pixel'], 'rightdown')
            v = v[:, :, y:y + ch, x:x + cw]
            v = torch.flip(v, dims=[-1]) if f else v
            isr.append(v.contiguous())
        chans.append(torch.cat(isr)[:, :1])
    return torch.cat(chans, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'isr3_bench.txt'))
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=20)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)

    def gray_of(B, H, W):
        base = torch.randint(0, 256, (B, H // 16 + 1, W // 16 + 1), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :H, :W]
        return (base * 0.8 + torch.randint(0, 52, (B, H, W), generator=g)).to(torch.uint8).contiguous().to(dev)
    prm = ops.isr_multi_params(PRESET, 'rightdown', dev)
    g512, gdz = gray_of(2, 512, 512), gray_of(2, 540, 960)
    wins = [(131, 7, 1), (400, 28, 0)]
    win = torch.tensor(wins, dtype=torch.int32).to(dev)
    assert torch.equal(ops.isr_multi(g512, VR, prm, 3), three_calls(g512))
    assert torch.equal(ops.isr_multi(gdz, VR, prm, 3, window=win, out_size=(512, 512)), loader_loop(gdz, wins, 512, 512))
    isr = (torch.rand(2, 3, 512, 512, generator=g) * 2 - 1).to(dev)
    taps, tf = (t.to(dev) for t in ops.cow_mask_params([dict(p=0.7, sigma=16.3, max_sigma=16), dict(p=0.7, sigma=16.8, max_sigma=16)]))
    lines = [f'Multi-parameter ISR and cow mask on {torch.cuda.get_device_name(0)}; median [min, max] us per call, {args.reps} x {args.inner} calls',
             f'{"case":58s} {"launches":>8s} {"us":>26s}']

    def row(name, launches, t):
        lines.append(f'{name:58s} {launches:8d} {t[0]:10.1f} [{t[1]:6.1f}, {t[2]:6.1f}]')
    a = timed(lambda: ops.isr_multi(g512, VR, prm, 3), args.reps, args.inner)
    b = timed(lambda: three_calls(g512), args.reps, args.inner)
    row('isr_multi [2,512,512] C=3', 3, a)
    row('  3 x isr_from_gray + pick + cat', 3 * 3 + 1, b)
    lines.append(f'  ratio composition / fused: {b[0] / a[0]:.2f}x')
    c = timed(lambda: ops.isr_multi(gdz, VR, prm, 3, window=win, out_size=(512, 512)), args.reps, args.inner)
    d = timed(lambda: loader_loop(gdz, wins, 512, 512), args.reps, args.inner)
    row('isr_multi [2,540,960] C=3, window 512 x 512 (one flipped)', 3, c)
    # per row and sample: 3 kernels + one copy (flip or contiguous); per row a cat; then the cat of the picks
    row('  per-sample loop x 3 rows (isr_from_gray, slice, flip, cat)', 3 * (2 * 4 + 1) + 1, d)
    lines.append(f'  ratio loop / fused: {d[0] / c[0]:.2f}x')
    e = timed(lambda: ops.cow_mask(isr, taps, tf, seed=1, offset=0), args.reps, args.inner)
    row('cow_mask [2,3,512,512] K=195, generated field', 3, e)
    must = 2 * isr.numel() * 4
    lines.append(f'  bytes it must move (ISR read + written): {must / 1e6:.2f} MB -> {must / e[0] / 1e3:.1f} GB/s effective; '
                 f'{2 * 2 * 512 * 512 * 195 * 2 / e[0] / 1e6:.2f} TFLOP/s of blur arithmetic')
    ok = a[0] <= b[0] and c[0] <= d[0]
    lines.append('expectation "the fused call is no slower than the composition it replaces": ' + ('holds' if ok else 'DOES NOT HOLD'))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
