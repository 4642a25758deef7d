#!/usr/bin/env python3
"""Benchmark of the validation tail: the shipped per-image path (up-sample(s) to 19 x H x W + soft-max + flip + argmax + host copy +
intersect_and_union: what `simple_test` + `mean_iou` do behind the network) against the fused on-device one (`ops.seg_predict` with the
confusion counters: one launch per image, nothing reaches the host before the end), in the same process on the same tensors, the two
alternating; then whole images through the full-depth fusion model in bf16 (`simple_test` + `mean_iou` against `predict` + meter).
Per-image times: the median over the repetitions of a window of `--images` images; `device` = HIP events around the window,
`wall` = host clock around the window including the synchronise that ends it.  Bytes/s of seg_predict = its algorithmic bytes
(logits read + labels written + ground truth read) over the device time.
Usage (GPU box): python tools/eval_bench.py [--reps 30] [--images 8] [--skip-model]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmda_amd.runtime as rt  # noqa: E402
from cmda_amd import metrics, ops, segmentors  # noqa: E402
from cmda_amd.registry import build_segmentor  # noqa: E402

NC = 19
TAILS = [   # (name, B, (h, w), (H, W), (OH, OW), flip)
    ('440x640 B=1', 1, (110, 160), (440, 640), (440, 640), 0),
    ('440x640 B=4', 4, (110, 160), (440, 640), (440, 640), 0),
    ('480x700 flip B=1', 1, (110, 160), (440, 640), (480, 700), 1),
]


def median(v):
    return sorted(v)[len(v) // 2]


def window(fn, images):
    """one timed window of `images` calls -> (device us, wall us) per call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(images):
        fn()
    e1.record()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return e0.elapsed_time(e1) / images * 1e3, (t1 - t0) / images * 1e6


def compare(paths, reps, images, warmup=3):
    """paths: {name: fn}; the windows of the paths alternate -> {name: (device median, wall median, wall min, wall max)}"""
    res = {k: [] for k in paths}
    for rep in range(warmup + reps):
        for k, fn in paths.items():
            w = window(fn, images)
            if rep >= warmup:
                res[k].append(w)
    return {k: (median([d for d, _ in v]), median([w for _, w in v]), min(w for _, w in v), max(w for _, w in v)) for k, v in res.items()}


def row(name, path, r, extra=''):
    print(f'{name:18s} {path:24s} device {r[0]:9.1f} us   wall {r[1]:9.1f} us [{r[2]:8.1f},{r[3]:9.1f}] per image-call{extra}', flush=True)


def bench_tails(reps, images, dev):
    for name, B, (h, w), (H, W), (OH, OW), flip in TAILS:
        g = torch.Generator().manual_seed(5)
        logits = (torch.randn(B, h, w, NC, generator=g) * 4).to(dev)
        gt_host = torch.randint(0, NC, (B, OH, OW), generator=g)
        gt_host[torch.rand(B, OH, OW, generator=g) < 0.1] = 255
        gt_np = [t.numpy() for t in gt_host]                    # the shipped path scores host label maps, image by image
        gt8 = gt_host.to(torch.uint8).to(dev)
        meta = dict(flip=bool(flip), flip_direction='horizontal')
        meter = metrics.ConfusionMeter(NC, 255, device=dev)
        tot = []

        def old_tail():
            seg = segmentors._resize_logits(ops.upsample_logits_nchw(logits, H, W), (OH, OW))
            maps = segmentors._label_maps(segmentors._flip_back(torch.softmax(seg, dim=1), meta))
            tot.append(metrics.total_intersect_and_union(maps, gt_np, NC, 255))
            return maps

        def new_tail():
            return ops.seg_predict(logits, H, W, (OH, OW), flip, gt8, meter.conf, 255)

        # same result first: labels and the four area vectors
        maps, labels = old_tail(), new_tail()
        differ = int((torch.as_tensor(maps[0]).to(dev) != labels[0]).sum()) if B == 1 else \
            int((torch.stack([torch.as_tensor(m) for m in maps]).to(dev) != labels).sum())
        same_areas = all(torch.equal(a.cpu(), b) for a, b in zip(meter.areas(), tot[0]))
        print(f'{name:18s} labels differing between the paths: {differ} of {labels.numel()}; areas equal: {same_areas}', flush=True)
        r = compare({'old': old_tail, 'new': new_tail}, reps, images)
        tot.clear()
        bytes_new = B * (h * w * NC * 4 + OH * OW * 2)
        row(name, 'old tail (host score)', r['old'])
        row(name, 'seg_predict + counters', r['new'], f'   {bytes_new / 1e6:.2f} MB -> {bytes_new / r["new"][0] / 1e3:.1f} GB/s   '
            f'device {r["old"][0] / r["new"][0]:.1f}x, wall {r["old"][1] / r["new"][1]:.1f}x')


def bench_model(reps, images, dev):
    dims = [64, 128, 320, 512]
    decoder = dict(embed_dims=256, embed_cfg=dict(type='mlp', act_cfg=None, norm_cfg=None),
                   embed_neck_cfg=dict(type='mlp', act_cfg=None, norm_cfg=None),
                   fusion_cfg=dict(type='aspp', sep=True, dilations=(1, 6, 12, 18), pool=False, act_cfg=dict(type='ReLU'),
                                   norm_cfg=dict(type='BN', requires_grad=True)),
                   train_type='cs2dsec_image+events_together', share_decoder=True)
    head = dict(type='DAFormerHeadFusion', in_channels=dims, in_index=[0, 1, 2, 3], channels=256, num_classes=NC, dropout_ratio=0.1,
                norm_cfg=dict(type='BN', requires_grad=True), align_corners=False, decoder_params=decoder,
                loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
    bbc = dict(type='mit_b5', style='pytorch', drop_path_rate=0.1)
    torch.manual_seed(7)
    model = build_segmentor(dict(type='FusionEncoderDecoder', backbone_image=dict(bbc), backbone_events=dict(bbc),
                                 fusion_module=dict(type='AttentionAvgFusion', in_channels=dims, drop_path_rate=0.1),
                                 decode_head=head, train_type='cs2dsec_image+events_together', test_cfg=dict(mode='whole')))
    model.init_weights()
    model.to(dev).eval()
    g = torch.Generator().manual_seed(9)
    samples = []
    for i in range(images):
        gt = torch.randint(0, NC, (440, 640), generator=g)
        gt[torch.rand(440, 640, generator=g) < 0.1] = 255
        samples.append(dict(warp_image=torch.randn(1, 3, 440, 640, generator=g).to(dev),
                            events_vg=torch.randn(1, 3, 440, 640, generator=g).clamp(-1, 1).to(dev),
                            img_metas=dict(ori_shape=(440, 640, 3), flip=bool(i % 2), flip_direction='horizontal'), gt=gt))
    rt.set_compute_dtype(torch.bfloat16)
    out = {}

    def old_pass():
        maps = [model.simple_test(True, **{k: v for k, v in s.items() if k != 'gt'})[0] for s in samples]
        out['old'] = metrics.mean_iou(maps, [s['gt'].numpy() for s in samples], NC, 255)

    gts = [s['gt'].to(torch.uint8).to(dev) for s in samples]     # (the loader's uint8 label maps, on the device)

    def new_pass():
        meter = metrics.ConfusionMeter(NC, 255, device=dev)
        for s, gt in zip(samples, gts):
            model.predict(True, gt_semantic_seg=gt, meter=meter, **{k: v for k, v in s.items() if k != 'gt'})
        out['new'] = {k: v.cpu() for k, v in meter.compute().items()}

    try:
        with torch.no_grad():
            # where the two paths' labels may differ at all: both tails on the logits of ONE forward pass (flipped sample), and whether a
            # second pass over the same input returns the same logits
            kw = {k: v for k, v in samples[1].items() if k != 'gt'}
            low = model.encode_decode_lowres(kw['warp_image'], kw['events_vg'], None, {'output_type': 'fusion'})['fusion_output']
            again = model.encode_decode_lowres(kw['warp_image'], kw['events_vg'], None, {'output_type': 'fusion'})['fusion_output']
            prob = segmentors._flip_back(torch.softmax(ops.upsample_logits_nchw(low, 440, 640), dim=1), kw['img_metas'])
            top2 = prob.topk(2, dim=1).values
            differ = prob.argmax(dim=1) != ops.seg_predict(low, 440, 640, None, 1)
            print(f'one forward pass, both tails: {int(differ.sum())} labels differ, {int((differ & (top2[:, 0] != top2[:, 1])).sum())} of them '
                  f'outside bitwise ties of the soft-max ({int((top2[:, 0] == top2[:, 1]).sum())} tied pixels); two passes over the same '
                  f'input bitwise equal: {torch.equal(low, again)}', flush=True)
            r = compare({'old': old_pass, 'new': new_pass}, max(5, reps // 4), 1, warmup=2)
    finally:
        rt.set_compute_dtype(torch.float32)
    name = f'fusion b5 bf16 x{images}'
    print(f'{name:18s} mIoU simple_test + mean_iou {out["old"]["mIoU"].item():.6f}, predict + meter {out["new"]["mIoU"].item():.6f}')
    per = lambda t: tuple(x / images for x in t)
    row(name, 'simple_test + mean_iou', per(r['old']))
    row(name, 'predict + meter', per(r['new']), f'   wall {r["old"][1] / r["new"][1]:.3f}x')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30, help='timed windows per path (at least 20); the median is reported')
    ap.add_argument('--images', type=int, default=8, help='image-calls per window')
    ap.add_argument('--skip-model', action='store_true', help='the tail alone')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('eval_bench.py measures on the GPU; none found')
    reps = max(20, args.reps)
    print(f'# {torch.cuda.get_device_name(0)}; {reps} windows of {args.images} image-calls per path after 3 warm-up windows, paths alternating')
    dev = torch.device('cuda:0')
    bench_tails(reps, args.images, dev)
    if not args.skip_model:
        bench_model(reps, args.images, dev)


if __name__ == '__main__':
    main()
