"""ms per training step of the image-only DACS types (DAFormer's DACS baseline: one MiT-B5, a plain DAFormerHead) at bench.py's
shape -- 512 x 512, 2 + 2 samples, bf16, hipGraph replay, overlapped optimizer update: 'cs2dsec_image' with the ImageNet feature
distance off and on (lambda 0.005, the classes and min ratio of configs/fusion/*), and 'cs2dz_image' with the 3 -> 3 day -> night
generator (seeded random weights); plus the generator's last layer (Conv2d(64, 3, 7) + Tanh on 2 x 512 x 512) as the stencil kernel
(cmda_conv_co3) against its implicit-GEMM form.  bench.py is not involved beyond its synthetic data and head settings.
Runs alternate `--rounds` times in one process; prints one JSON line.

    python tools/image_uda_step_bench.py --steps 30 --warmup 5 --rounds 2
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

FD = dict(imnet_feature_dist_lambda=0.005, imnet_feature_dist_classes=[6, 7, 11, 12, 13, 14, 15, 16, 17, 18],
          imnet_feature_dist_scale_min_ratio=0.75)


def image_cfg(train_type, lam=0.0, generator=False):
    """the image-only counterpart of bench.dacs_cfg: EventsEncoderDecoder (mit_b5, DAFormerHead) under the same DACS settings"""
    head = dict(type='DAFormerHead', dropout_ratio=0.1, decoder_params=dict(bench.DECODER), **bench.HEAD_CFG)
    model = dict(type='EventsEncoderDecoder', backbone=dict(type='mit_b5', style='pytorch', drop_path_rate=0.1), decode_head=head,
                 train_cfg=dict(), test_cfg=dict(mode='whole'))
    uda = dict(type='DACS', alpha=0.999, pseudo_threshold=0.968, pseudo_weight_ignore_top=0, pseudo_weight_ignore_bottom=0,
               imnet_feature_dist_lambda=0, imnet_feature_dist_classes=None, imnet_feature_dist_scale_min_ratio=None, mix='class',
               blur=True, color_jitter_strength=0.2, color_jitter_probability=0.2, debug_img_interval=1000, print_grad_magnitude=False,
               train_type=train_type, forward_cfg=dict(), cyclegan_id2in_path='random' if generator else '', sky_mask=None)
    if lam > 0:
        uda.update(FD, imnet_feature_dist_lambda=lam)
    return dict(model=model, uda=uda, runner=dict(type='IterBasedRunner', max_iters=40000))


def run(train_type, lam, generator, steps, warmup, dev):
    import cmda_amd.runtime as rt
    from cmda_amd import optim
    from cmda_amd.registry import build_train_model
    rt.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(1234)
    dacs = build_train_model(image_cfg(train_type, lam, generator))
    dacs.init_weights()
    dacs.to(dev).train()
    opt = optim.FlatAdamW(dacs.model, lr=6e-5, weight_decay=0.01, custom_keys=bench.CUSTOM_KEYS)
    opt.overlap = True
    dacs.attach_flat_store(opt)
    pairs = bench.synthetic_pairs(2, 512, 100, dev)
    src = dict(image=pairs['source']['image'], label=pairs['source']['label'])
    tgt = {('warp_image' if train_type == 'cs2dsec_image' else 'image'): pairs['target']['warp_image']}
    batch = dict(source=src, target=tgt)
    torch.manual_seed(1000)
    np.random.seed(1000)
    dacs.enable_graph(warmup_iters=2)
    it = [0]

    def step():
        opt.zero_grad()
        lv = dacs(**batch)
        opt.step(optim.poly_warm_scale(it[0]))
        it[0] += 1
        return lv

    for _ in range(3 + warmup):
        step()
    opt.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        lv = step()
    opt.synchronize()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    assert dacs._graph is not None
    out = dict(ms_per_step=round(ms, 3), losses={k: round(float(v), 5) for k, v in lv.items() if 'loss' in k})
    del dacs, opt
    torch.cuda.empty_cache()
    return out


def last_layer(dev, reps=50):
    """the 3 -> 3 generator's last layer on 2 x 512 x 512: stencil kernel vs implicit GEMM (N = 3 on a 64-wide tile), bf16"""
    import cmda_amd.runtime as rt
    from cmda_amd import ops
    from cmda_amd.ops import conv_view, plain_view
    rt.set_compute_dtype(torch.bfloat16)
    B, H, W, C = 2, 512, 512, 64
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B * H * W, C, generator=g).to(torch.bfloat16).to(dev)
    wt = (torch.randn(3, 7 * 7 * C, generator=g) * 0.02).to(torch.bfloat16).to(dev)
    bias = torch.zeros(3, device=dev)
    scale, shift = torch.ones(3, device=dev), torch.zeros(3, device=dev)
    y = torch.empty(B * H * W, 3, dtype=torch.float32, device=dev)

    def stencil():
        return ops.conv_co3(x, wt, bias, B, H, W, C, 7, 3, True, 'tanh', scale, shift)

    def gemm():
        ops.gemm(conv_view(x, B, H, W, C, 7, 7, 1, 3, 1, OH=H, OW=W, reflect=1), plain_view(wt, 3, 49 * C), y, B * H * W, 3, 49 * C,
                 dtype=rt.tag(), bias=bias, act='tanh')
        return y

    out = {}
    for name, fn in (('stencil', stencil), ('gemm', gemm)):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[f'{name}_us'] = round(e0.elapsed_time(e1) * 1e3 / reps, 2)
    a = stencil()
    b = gemm().view(B, H, W, 3).permute(0, 3, 1, 2)
    out['max_abs_diff'] = float((a - b).abs().max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=2)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    cases = {'dsec_fd_off': ('cs2dsec_image', 0.0, False), 'dsec_fd_on': ('cs2dsec_image', FD['imnet_feature_dist_lambda'], False),
             'dz_generator': ('cs2dz_image', 0.0, True)}
    runs = {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, (tt, lam, gen) in cases.items():
            runs[k].append(run(tt, lam, gen, args.steps, args.warmup, dev))
    best = {f'{k}_ms': min(r['ms_per_step'] for r in v) for k, v in runs.items()}
    print(json.dumps(dict(workload='image-only DACS, MiT-B5, 512x512, 2+2, bf16, hipGraph replay, overlapped update', steps=args.steps,
                          warmup=args.warmup, **best, last_layer=last_layer(dev), runs=runs)))


if __name__ == '__main__':
    main()
