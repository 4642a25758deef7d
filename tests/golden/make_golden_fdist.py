"""Generates the ImageNet feature-distance fixtures from the reference's OWN code (imported unmodified through ref_shim, with
make_golden's helpers): downscale_label.npz (mmseg/utils/utils.py:18-39 downscale_label_ratio + calc_feat_dist's class mask),
dacs_step_fdist.npz (DACS.train_step with imnet_feature_dist_lambda = 0.005, dacs.py:328-354 / :566-577, iterations 0-1) and
dacs_fdist_keys.json (the DACS state-dict keys with the frozen ImageNet model).  Runs only in the authoring container.
Usage: python tests/golden/make_golden_fdist.py [case ...]
"""
import json
import os
import random
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import ref_shim  # noqa: E402
from weights import DACS_SEG_SCALE, dacs_batch, seeded_fill  # noqa: E402

FD_CLASSES = [6, 7, 11, 12, 13, 14, 15, 16, 17, 18]   # configs/fusion/*.py
FD_RATIO = 0.75
FD_LAMBDA = 0.005
FD_SEEDS = dict(imnet=114, label=115)
CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def crafted_label(B, H, W, s, seed, n_classes=19):
    """cell-aligned label: per s x s cell a majority class at a drawn ratio (pure, exactly 3/4, just below 3/4, a half-half tie,
    a mixed cell) or an ignore majority; the rest of the cell from other classes"""
    g = torch.Generator().manual_seed(seed)
    lab = torch.empty(B, 1, H, W, dtype=torch.int64)
    kinds = ['pure', 'r768', 'r767', 'tie', 'mixed', 'ignore']
    n = s * s
    for b in range(B):
        for i in range(H // s):
            for j in range(W // s):
                kind = kinds[int(torch.randint(0, len(kinds), (1,), generator=g))]
                major = int(torch.randint(0, n_classes, (1,), generator=g))
                other = (major + 1 + int(torch.randint(0, n_classes - 1, (1,), generator=g))) % n_classes
                cell = torch.full((n,), major, dtype=torch.int64)
                if kind == 'r768':
                    cell[n * 3 // 4:] = other
                elif kind == 'r767':
                    cell[n * 3 // 4 - 1:] = other
                elif kind == 'tie':
                    cell[n // 2:] = other
                elif kind == 'mixed':
                    cell = torch.randint(0, n_classes, (n,), generator=g)
                elif kind == 'ignore':
                    cell[: n * 5 // 8] = 255
                    cell[n * 5 // 8:] = other
                cell = cell[torch.randperm(n, generator=g)]
                lab[b, 0, i * s:(i + 1) * s, j * s:(j + 1) * s] = cell.view(s, s)
    return lab


@case
def downscale_label():
    U = ref_shim.load('mmseg.utils.utils')
    out = {}
    fdc = torch.tensor(FD_CLASSES)
    for s in (2, 4, 8, 32):
        H, W = (4 * s, 6 * s) if s < 32 else (64, 128)
        lab = crafted_label(2, H, W, s, 1000 + s)
        out[f's{s}.label'] = lab.to(torch.uint8)
        for r in (0.75, 0.5, 0.25):
            resc = U.downscale_label_ratio(lab, s, r, 19, 255).long()
            mask = torch.any(resc[..., None] == fdc, -1)
            out[f's{s}.r{int(r * 100)}.rescaled'] = resc.to(torch.uint8)
            out[f's{s}.r{int(r * 100)}.mask'] = mask
    out['classes'] = np.array(FD_CLASSES)
    mg.save('downscale_label', **out)


def fdist_cfg(G_path, lam):
    cfg = mg.dacs_cfg(G_path)
    cfg.update(imnet_feature_dist_lambda=lam, imnet_feature_dist_classes=list(FD_CLASSES), imnet_feature_dist_scale_min_ratio=FD_RATIO)
    return cfg


def _reference_dacs(lam):
    """make_golden.dacs_step's set-up: the reference DACS at the fixture width (student / teacher / generator seeds, peaky
    classifier), plus the ImageNet model filled from its own seed"""
    import torch.nn as nn
    nn.Module.cuda = lambda self, *a, **k: self
    mm = sys.modules['mmseg.models']
    for k in ('BaseSegmentor', 'BaseSegmentorEvents', 'BaseSegmentorFusion'):
        setattr(mm, k, getattr(mg.ns.seg_base, k))
    cg = sys.modules['mmseg.models.cyclegan']
    cg.define_G, cg.LightNet = mg.ns.cyclegan.define_G, getattr(mg.ns.cyclegan, 'LightNet', None)
    D = ref_shim.load('mmseg.models.uda.dacs')
    G = mg.ns.cyclegan.define_G()
    seeded_fill(G, 113)
    gpath = os.path.join(tempfile.mkdtemp(), 'G.pth')
    torch.save(G.state_dict(), gpath)
    dacs = D.DACS(**fdist_cfg(gpath, lam))
    seeded_fill(dacs.model, 111)
    seeded_fill(dacs.ema_model, 112)
    if dacs.imnet_model is not None:
        seeded_fill(dacs.imnet_model, FD_SEEDS['imnet'])
    with torch.no_grad():
        dacs.model.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE)
    dacs.train()

    class _NoPlot:
        def __getattr__(self, n):
            if n.startswith('__'):
                raise AttributeError(n)
            if n == 'subplots':
                axs = np.empty((8, 8), dtype=object)
                for i in range(8):
                    for j in range(8):
                        axs[i, j] = _NoPlot()
                return lambda *a, **k: (_NoPlot(), axs)
            return _NoPlot()

        def __call__(self, *a, **k):
            return _NoPlot()
    D.plt, D.subplotimg = _NoPlot(), (lambda *a, **k: None)
    return dacs


GATES = [(0.13, 0.31, 0.5), (0.07, 0.44, 0.9)]   # (colour-jitter u <= p = 0.2: off, blur u <= 0.5: off, sigma)


def fdist_batch():
    src, tg = dacs_batch()
    src['label'] = crafted_label(1, 512, 512, 32, FD_SEEDS['label'])
    return src, tg


def _step(dacs, opt, src, tg, it):
    seq = iter(GATES[it])
    uniform = random.uniform
    random.uniform = lambda a, b: next(seq)
    torch.manual_seed(600 + it)
    np.random.seed(600 + it)
    classes = torch.unique(src['label'])
    n = classes.shape[0]
    st = np.random.get_state()
    chosen = classes[torch.Tensor(np.random.choice(n, int((n + n % 2) / 2), replace=False)).long()]
    np.random.set_state(st)
    batch = dict(source={k: v.clone() for k, v in src.items()}, target={k: v.clone() for k, v in tg.items()})
    try:
        res = dacs.train_step(batch, opt)
    finally:
        random.uniform = uniform
    return res, chosen


@case
def dacs_step_fdist():
    src, tg = fdist_batch()
    out = {'label': src['label'].to(torch.uint8)}
    # iteration 0 from the same state with lambda = 0 and lambda = 0.5: the image encoder's FD gradient in isolation
    for tag, lam in (('lam0', 0.0), ('lam05', 0.5)):
        dacs = _reference_dacs(lam)
        opt = torch.optim.AdamW(dacs.model.parameters(), lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01)
        _step(dacs, opt, src, tg, 0)
        for k, p in dacs.model.named_parameters():
            if k.startswith('backbone_image.'):
                out[f'{tag}.grad.{k}'] = mg.fingerprint(p.grad)
    dacs = _reference_dacs(FD_LAMBDA)
    opt = torch.optim.AdamW(dacs.model.parameters(), lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01)
    for it in range(2):
        res, chosen = _step(dacs, opt, src, tg, it)
        lv = res['log_vars']
        mask = dacs.debug_fdist_mask
        if it == 0:
            assert 0 < int(mask.sum()) < mask.numel(), int(mask.sum())
        out[f'it{it}.losses'] = np.array([lv['decode.loss_seg'], lv['decode.acc_seg'], lv['mix.decode.loss_seg'], lv['mix.decode.acc_seg'],
                                          lv['src.loss_imnet_feat_dist']])
        out[f'it{it}.choice'] = float(dacs.forward_cfg['isr_events_fusion_choice'])
        out[f'it{it}.gates'] = np.array(GATES[it])
        out[f'it{it}.classes'] = chosen
        out[f'it{it}.fdist_mask'] = mask
        out[f'it{it}.gt_rescale'] = dacs.debug_gt_rescale.to(torch.uint8)
        for k, p in dacs.model.named_parameters():
            out[f'it{it}.grad.{k}'] = mg.fingerprint(p.grad)
            out[f'it{it}.param.{k}'] = mg.fingerprint(p.data)
        print('iteration', it, lv, 'mask', int(mask.sum()), 'of', mask.numel())
    for k, p in dacs.imnet_model.named_parameters():
        out[f'imnet.{k}'] = mg.fingerprint(p.data)
    mg.save('dacs_step_fdist', **out)
    keys = list(dacs.state_dict().keys())
    with open(os.path.join(HERE, 'dacs_fdist_keys.json'), 'w') as f:
        json.dump(keys, f, indent=0)
        f.write('\n')
    print('wrote dacs_fdist_keys', len(keys), sum(k.startswith('imnet_model.') for k in keys))


if __name__ == '__main__':
    for n in sys.argv[1:] or list(CASES):
        print('==', n)
        CASES[n]()
