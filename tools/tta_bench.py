#!/usr/bin/env python3
"""Benchmark of the sliding-window and multi-view evaluation tails (seg_tta.hip) against the composition of the ops that existed
before them, in the same process on the same tensors, the two alternating:
 (a) the tail alone, from given low-resolution logits
     slide : 1024 x 2048, crop 1024^2, stride 768^2 (3 windows), nc = 19: per-window upsample_logits_nchw + pad + add + divide + argmax
             against one ops.seg_predict_windows launch;
     views : 440 x 640 whole, the ratios 0.5 ... 1.75 x flip (12 views): per view up-sample + resize + soft-max + flip + add, then
             divide + argmax, against 12 ops.seg_prob_accumulate launches + one ops.prob_predict launch;
 (b) images per second through the full-depth fusion model in bf16 under test_cfg.mode 'slide' (512 x 1024, crop 512^2, stride 384^2:
     3 windows): all windows as one batch (slide_batch=None) against the reference's loop (slide_batch=1).
Per-call times: the median over the repetitions of a window of `--calls` calls; `device` = HIP events around the window, `wall` = host
clock around the window including the synchronise that ends it.  GB/s = algorithmic bytes over the device time.
Usage (GPU box): python tools/tta_bench.py [--reps 30] [--calls 4] [--skip-model] [--out profiles/tta_bench.txt]"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import cmda_amd.runtime as rt  # noqa: E402
from cmda_amd import ops, segmentors  # noqa: E402
from cmda_amd.registry import build_segmentor  # noqa: E402
from eval_bench import compare  # noqa: E402

NC = 19
RATIOS = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def row(name, path, r, extra=''):
    say(f'{name:22s} {path:34s} device {r[0]:9.1f} us   wall {r[1]:9.1f} us [{r[2]:8.1f},{r[3]:9.1f}] per call{extra}')


def bench_slide_tail(reps, calls, dev):
    H, W, crop, stride = 1024, 2048, (1024, 1024), (768, 768)
    wins = ops.slide_windows(H, W, crop, stride)
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(len(wins), 1, 256, 256, NC, generator=g) * 4).to(dev)

    def old_tail():
        preds = torch.zeros(1, NC, H, W, device=dev)
        count = torch.zeros(1, 1, H, W, device=dev)
        for k, (y1, x1, y2, x2) in enumerate(wins):
            preds += F.pad(ops.upsample_logits_nchw(logits[k], y2 - y1, x2 - x1), (x1, W - x2, y1, H - y2))
            count[:, :, y1:y2, x1:x2] += 1
        return (preds / count).argmax(dim=1)

    def new_tail():
        return ops.seg_predict_windows(logits, H, W, crop, stride)
    a, b = old_tail(), new_tail()
    name = f'slide {H}x{W} K={len(wins)}'
    say(f'{name:22s} labels differing between the paths: {int((a != b).sum())} of {b.numel()}')
    r = compare({'old': old_tail, 'new': new_tail}, reps, calls)
    nbytes = logits.numel() * 4 + H * W
    row(name, 'composition of existing ops', r['old'])
    row(name, 'seg_predict_windows', r['new'], f'   {nbytes / 1e6:.2f} MB -> {nbytes / r["new"][0] / 1e3:.1f} GB/s   '
        f'device {r["old"][0] / r["new"][0]:.2f}x, wall {r["old"][1] / r["new"][1]:.2f}x')


def bench_views_tail(reps, calls, dev):
    OH, OW = 440, 640
    g = torch.Generator().manual_seed(6)
    views = []
    for ratio in RATIOS:
        H, W = int(OH * ratio + 0.5), int(OW * ratio + 0.5)
        for flip in (0, 1):
            views.append(((torch.randn(1, (H + 3) // 4, (W + 3) // 4, NC, generator=g) * 4).to(dev), H, W, flip))
    acc = torch.empty(1, NC, OH, OW, device=dev)

    def old_tail():
        seg = None
        for lg, H, W, flip in views:
            p = torch.softmax(segmentors._resize_logits(ops.upsample_logits_nchw(lg, H, W), (OH, OW)), dim=1)
            p = p.flip(dims=(3,)) if flip else p
            seg = p if seg is None else seg.add_(p)
        seg /= len(views)
        return seg.argmax(dim=1)

    def accumulate():
        for i, (lg, H, W, flip) in enumerate(views):
            ops.seg_prob_accumulate(lg[None], H, W, (H, W), (H, W), (OH, OW), flip, acc, i > 0)

    def new_tail():
        accumulate()
        return ops.prob_predict(acc, len(views))
    a, b = old_tail(), new_tail()
    name = f'views {OH}x{OW} n={len(views)}'
    say(f'{name:22s} labels differing between the paths: {int((a != b).sum())} of {b.numel()}')
    r = compare({'old': old_tail, 'new': new_tail, 'acc': accumulate, 'pred': lambda: ops.prob_predict(acc, len(views))}, reps, calls)
    plane = NC * OH * OW * 4
    b_acc = sum(v[0].numel() * 4 for v in views) + plane * (2 * len(views) - 1)
    b_pred = plane + OH * OW
    row(name, 'composition of existing ops', r['old'])
    row(name, 'seg_prob_accumulate x n + prob_predict', r['new'], f'   device {r["old"][0] / r["new"][0]:.2f}x, wall {r["old"][1] / r["new"][1]:.2f}x')
    row(name, '  seg_prob_accumulate x n alone', r['acc'], f'   {b_acc / 1e6:.2f} MB -> {b_acc / r["acc"][0] / 1e3:.1f} GB/s')
    row(name, '  prob_predict alone', r['pred'], f'   {b_pred / 1e6:.2f} MB -> {b_pred / r["pred"][0] / 1e3:.1f} GB/s')


def bench_model(reps, dev):
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
                                 decode_head=head, train_type='cs2dsec_image+events_together',
                                 test_cfg=dict(mode='slide', crop_size=(512, 512), stride=(384, 384))))
    model.init_weights()
    model.to(dev).eval()
    g = torch.Generator().manual_seed(9)
    kw = dict(warp_image=torch.randn(1, 3, 512, 1024, generator=g).to(dev), events_vg=torch.randn(1, 3, 512, 1024, generator=g).clamp(-1, 1).to(dev),
              img_metas=dict(ori_shape=(512, 1024, 3), flip=False))
    rt.set_compute_dtype(torch.bfloat16)

    def run(slide_batch):
        def fn():
            model.slide_batch = slide_batch
            return model.predict(True, **kw)
        return fn
    try:
        with torch.no_grad():
            a, b = run(None)(), run(1)()
            r = compare({'batch': run(None), 'loop': run(1)}, max(5, reps // 4), 1, warmup=2)
    finally:
        rt.set_compute_dtype(torch.float32)
        model.slide_batch = None
    name = 'fusion b5 bf16 512x1024'
    say(f'{name:22s} labels differing between slide_batch=None and slide_batch=1: {int((a != b).sum())} of {b.numel()}')
    row(name, 'slide_batch=1 (one window per pass)', r['loop'], f'   {1e6 / r["loop"][1]:.2f} images/s')
    row(name, 'slide_batch=None (3 windows, one pass)', r['batch'], f'   {1e6 / r["batch"][1]:.2f} images/s   wall {r["loop"][1] / r["batch"][1]:.3f}x')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30, help='timed windows per path (at least 20); the median is reported')
    ap.add_argument('--calls', type=int, default=4, help='calls per window')
    ap.add_argument('--skip-model', action='store_true', help='the tails alone')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tta_bench.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tta_bench.py measures on the GPU; none found')
    reps = max(20, args.reps)
    say(f'# {torch.cuda.get_device_name(0)}; {reps} windows of {args.calls} calls per path after 3 warm-up windows, paths alternating')
    dev = torch.device('cuda:0')
    bench_slide_tail(reps, args.calls, dev)
    bench_views_tail(reps, args.calls, dev)
    if not args.skip_model:
        bench_model(reps, dev)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
