"""Times the ISR augmentation ops (ops.sky_mask, ops.isr_noise with generated fields, ops.randn_fields) at 2 x 512 x 512 against the
torch composition of the same ops on the device (max_pool2d, avg_pool2d, interpolate, randn_like, indexing -- the reference's
sky_mask_transform / add_noise_on_isr with the host reads taken out, batched where torch can batch them), and writes
profiles/isr_aug_bench.txt.  Each timing is the median of `--reps` CUDA-event intervals over `--inner` back-to-back calls.

    python tools/isr_aug_bench.py [--out profiles/isr_aug_bench.txt]
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

B, C, H, W = 2, 3, 512, 512


def timed(fn, reps, inner):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def torch_sky_mask(label, isr, bank, draws):
    """sky_mask_transform per sample (the kernel size differs per sample) without its .item() / nonzero reads"""
    out = []
    for b, d in enumerate(draws):
        sky = (label[b:b + 1] == 10).float()
        k = d['k']
        x = isr[b] * (1 - sky)
        expansion = F.max_pool2d(sky, kernel_size=k, stride=1, padding=k // 2)
        weight = F.avg_pool2d(sky, kernel_size=k, stride=1, padding=k // 2) * torch.logical_not(sky)
        mx, mn = torch.max(weight), torch.min(weight)
        weight = (weight - mn) / (mx - mn)
        blur_w = 1 - torch.clamp(weight + d['lam'] * (weight != 0), min=0, max=1)
        noise = (bank[d['index']] / 128 - 1)[d['rows_dev']][:, d['cols_dev']]
        out.append(torch.clamp(x * blur_w + noise * expansion * d['intensity'], min=-1, max=1))
    return torch.stack(out)


def torch_isr_noise(isr, draws):
    """add_noise_on_isr batched over the samples that share the blur decision (here: all blurred), with randn_like fields"""
    x = isr[:, 0:1]
    x = F.interpolate(F.avg_pool2d(x, kernel_size=(2, 2)), size=x.shape[-2:], mode='bilinear', align_corners=False)
    t1, t2, inten = draws
    x = x * (torch.abs(torch.randn_like(x)) < t1)
    x = x + torch.randn_like(x) * inten * (torch.abs(torch.randn_like(x)) < t2)
    return torch.clamp(x, min=-1, max=1).repeat(1, 3, 1, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'isr_aug_bench.txt'))
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=20)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    label = torch.randint(0, 19, (B, H // 16, W // 16), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2).to(dev)
    isr = (torch.rand(B, C, H, W, generator=g) * 2 - 1).to(dev)
    bank = torch.randint(0, 256, (4, H, W), generator=g, dtype=torch.uint8).to(dev)
    torch.manual_seed(0)
    draws = [ops.draw_sky_mask(4, H, W) for _ in range(B)]
    for d, k in zip(draws, (31, 61)):
        d['k'] = k
        d['rows_dev'], d['cols_dev'] = d['rows'].long().to(dev), d['cols'].long().to(dev)
    prm, rows, cols = (t.to(dev) for t in ops.sky_mask_params(draws))
    nprm = ops.isr_noise_params([(1, 1.2, 0.5, 0.2)] * B).to(dev)
    rows_out = []
    cases = [('sky_mask (k = 31, 61)', lambda: ops.sky_mask(label, isr, bank, prm, rows, cols), lambda: torch_sky_mask(label, isr, bank, draws)),
             ('isr_noise noise+blur, generated fields', lambda: ops.isr_noise(isr, nprm, 'noise+blur', seed=1, offset=0),
              lambda: torch_isr_noise(isr, (1.2, 0.5, 0.2))),
             ('randn_fields (3 fields)', lambda: ops.randn_fields(B, H, W, 1, 0, device=dev),
              lambda: (torch.randn(B, H, W, device=dev), torch.randn(B, H, W, device=dev), torch.randn(B, H, W, device=dev)))]
    lines = [f'ISR augmentation ops at {B} x {C} x {H} x {W} on {torch.cuda.get_device_name(0)}; median [min, max] us per call, '
             f'{args.reps} x {args.inner} calls', f'{"op":44s} {"HIP us":>24s} {"torch composition us":>28s}  ratio']
    ok = True
    for name, ours, theirs in cases:
        a, t = timed(ours, args.reps, args.inner), timed(theirs, args.reps, args.inner)
        ok &= a[0] <= t[0]
        lines.append(f'{name:44s} {a[0]:8.1f} [{a[1]:6.1f}, {a[2]:6.1f}] {t[0]:12.1f} [{t[1]:6.1f}, {t[2]:6.1f}]  {t[0] / a[0]:5.2f}x')
        rows_out.append((name, a, t))
    lines.append('expectation "each op at or below the torch composition\'s time": ' + ('holds' if ok else 'DOES NOT HOLD'))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
