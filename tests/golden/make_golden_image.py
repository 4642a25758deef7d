"""Generates the fixtures of the image-only DACS train types 'cs2dsec_image' / 'cs2dz_image' from the reference's OWN code (imported
unmodified through ref_shim, with make_golden's helpers): dacs_step_image.npz (DACS.train_step, image-only branch of dacs.py:363-377,
:467-468, :569-570, :597-600, :719-791, with and without the ImageNet feature distance, and 'cs2dz_image' with the 3 -> 3 day -> night
generator of :105-113, :368-372), generator_33.npz (that generator's forward on its own), image_simple_test.npz
(EventsEncoderDecoder.simple_test at 440 x 640, encoder_decoder.py:525-603) and dacs_image_keys.json (the DACS state-dict keys, ImageNet
model included).  Runs only in the authoring container.
Usage: python tests/golden/make_golden_image.py [case ...]
"""
import json
import os
import random
import sys
import tempfile
from functools import partial

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import ref_shim  # noqa: E402
from make_golden_fdist import crafted_label  # noqa: E402
from weights import DACS_CH, DACS_DIMS, DACS_SEG_SCALE, dacs_batch, seeded_fill, seeded_randn  # noqa: E402

FD_CLASSES = [6, 7, 11, 12, 13, 14, 15, 16, 17, 18]   # configs/fusion/*.py
FD_RATIO = 0.75
FD_LAMBDA = 0.005
SEEDS = dict(student=121, teacher=122, imnet=124, generator=123, label=125, g33=131, simple=141)
FP_N = 16   # samples per fingerprint
GATES = [(0.13, 0.31, 0.5), (0.07, 0.44, 0.9), (0.18, 0.12, 0.3)]   # (colour-jitter u <= p = 0.2: off, blur u <= 0.5: off, sigma)
CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def image_model_cfg():
    """reduced-width EventsEncoderDecoder (one MiT, plain DAFormerHead) at the widths of the fusion fixtures"""
    bb = dict(type='MixVisionTransformer', patch_size=4, embed_dims=DACS_DIMS, num_heads=[1, 2, 5, 8], mlp_ratios=[4, 4, 4, 4],
              qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), depths=[1, 1, 1, 1], sr_ratios=[8, 4, 2, 1],
              drop_path_rate=0.0)
    head = dict(type='DAFormerHead', in_channels=DACS_DIMS, in_index=[0, 1, 2, 3], channels=DACS_CH, dropout_ratio=0.0,
                num_classes=19, norm_cfg=dict(type='BN', requires_grad=True), align_corners=False,
                decoder_params=dict(embed_dims=DACS_CH, embed_cfg=dict(type='mlp', act_cfg=None, norm_cfg=None),
                                    embed_neck_cfg=dict(type='mlp', act_cfg=None, norm_cfg=None),
                                    fusion_cfg=dict(type='aspp', sep=True, dilations=(1, 6, 12, 18), pool=False,
                                                    act_cfg=dict(type='ReLU'), norm_cfg=dict(type='BN', requires_grad=True))),
                loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
    return dict(type='EventsEncoderDecoder', pretrained=None, backbone=bb, decode_head=head,
                train_cfg=dict(work_dir='/tmp/cmda_golden_image'), test_cfg=dict(mode='whole'))


def image_cfg(train_type, lam, G_path=''):
    cfg = dict(model=image_model_cfg(), max_iters=40000, alpha=0.999, pseudo_threshold=0.968, pseudo_weight_ignore_top=0,
               pseudo_weight_ignore_bottom=0, imnet_feature_dist_lambda=lam, imnet_feature_dist_classes=list(FD_CLASSES),
               imnet_feature_dist_scale_min_ratio=FD_RATIO, mix='class', blur=True, color_jitter_strength=0.2,
               color_jitter_probability=0.2, debug_img_interval=10 ** 9, print_grad_magnitude=False, train_type=train_type,
               forward_cfg=dict(), img_self_res_reg='no', sky_mask=None)
    if G_path:
        cfg['cyclegan_id2in_path'] = G_path
    return cfg


def _reference_dacs(train_type, lam, with_G=False):
    nn.Module.cuda = lambda self, *a, **k: self
    torch.Tensor.cuda = lambda self, *a, **k: self
    mm = sys.modules['mmseg.models']
    for k in ('BaseSegmentor', 'BaseSegmentorEvents', 'BaseSegmentorFusion'):
        setattr(mm, k, getattr(mg.ns.seg_base, k))
    cg = sys.modules['mmseg.models.cyclegan']
    cg.define_G, cg.LightNet = mg.ns.cyclegan.define_G, getattr(mg.ns.cyclegan, 'LightNet', None)
    D = ref_shim.load('mmseg.models.uda.dacs')
    gpath = ''
    if with_G:
        G = mg.ns.cyclegan.define_G(input_nc=3, output_nc=3)
        seeded_fill(G, SEEDS['generator'])
        gpath = os.path.join(tempfile.mkdtemp(), 'G33.pth')
        torch.save(G.state_dict(), gpath)
    dacs = D.DACS(**image_cfg(train_type, lam, gpath))
    seeded_fill(dacs.model, SEEDS['student'])
    seeded_fill(dacs.ema_model, SEEDS['teacher'])
    if dacs.imnet_model is not None:
        seeded_fill(dacs.imnet_model, SEEDS['imnet'])
    with torch.no_grad():   # a peaky classifier: some pixels must clear the 0.968 confidence threshold
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


def image_batch(train_type):
    """dacs_batch's source image, the feature-distance fixture's cell-aligned label (some 32 x 32 cells pass the 0.75 class ratio: a
    non-empty feature-distance mask); the target image under the key of the train type (DSEC: warp_image, Dark Zurich: image)"""
    src, tg = dacs_batch()
    src = dict(image=src['image'], label=crafted_label(1, 512, 512, 32, SEEDS['label']))
    tg = dict(warp_image=tg['warp_image']) if train_type == 'cs2dsec_image' else dict(image=tg['warp_image'])
    return src, tg


def _run(tag, train_type, lam, iters, out, with_G=False):
    dacs = _reference_dacs(train_type, lam, with_G)
    opt = torch.optim.AdamW(dacs.model.parameters(), lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01)
    src, tg = image_batch(train_type)
    model, ema = dacs.get_model(), dacs.get_ema_model()
    captured = {}
    orig_ft, orig_ed = model.forward_train, ema.encode_decode

    def ft(image, events, gt, seg_weight=None, return_feat=False):
        if seg_weight is None:
            captured['src_img'] = image.detach().clone()
        else:
            captured.update(mixed_img=image.detach().clone(), mixed_lbl=gt.detach().clone(), mixed_weight=seg_weight.detach().clone())
        return orig_ft(image, events, gt, seg_weight=seg_weight, return_feat=return_feat)

    def ed(*a, **k):
        o = orig_ed(*a, **k)
        captured['teacher'] = o.detach().clone()
        return o
    model.forward_train, ema.encode_decode = ft, ed
    uniform = random.uniform
    for it in range(iters):
        seq = iter(GATES[it])
        random.uniform = lambda a, b: next(seq)
        torch.manual_seed(700 + it)
        np.random.seed(700 + it)
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
        lv = res['log_vars']
        names = ['decode.loss_seg', 'decode.acc_seg', 'mix.decode.loss_seg', 'mix.decode.acc_seg'] + (['src.loss_imnet_feat_dist'] if lam else [])
        prob, plabel = torch.max(torch.softmax(captured['teacher'], dim=1), dim=1)
        p = f'{tag}.it{it}'
        out[f'{p}.losses'] = np.array([lv[k] for k in names])
        out[f'{p}.log_keys'] = np.array(sorted(lv.keys()))
        out[f'{p}.gates'] = np.array(GATES[it])
        out[f'{p}.classes'] = chosen
        out[f'{p}.pseudo_label_s'] = plabel[..., ::8, ::8].to(torch.uint8)
        out[f'{p}.pseudo_conf'] = (prob >= 0.968).sum()
        out[f'{p}.teacher_s'] = captured['teacher'][..., ::64, ::64]
        out[f'{p}.mixed_img_s'] = captured['mixed_img'][..., ::16, ::16]
        out[f'{p}.mixed_lbl_s'] = captured['mixed_lbl'][..., ::8, ::8].to(torch.uint8)
        out[f'{p}.mixed_weight_s'] = captured['mixed_weight'][..., ::8, ::8]
        if lam:
            mask = dacs.debug_fdist_mask
            assert 0 < int(mask.sum()) < mask.numel(), int(mask.sum())
            out[f'{p}.fdist_mask_sum'] = mask.sum()
        if with_G:
            out[f'{p}.src_img_s'] = captured['src_img'][..., ::16, ::16]
        # fingerprints (FP_N samples + sum + abs-sum) of every student gradient and EMA weight, one row per parameter in the order of
        # `param_names` (one array per kind: a file of thousands of small entries is mostly zip headers)
        names = [k for k, _ in dacs.model.named_parameters()]
        assert names == [k for k, _ in dacs.ema_model.named_parameters()]
        out.setdefault('param_names', np.array(names))
        assert list(out['param_names']) == names
        out[f'{p}.grad'] = torch.stack([mg.fingerprint(q.grad, FP_N) for q in dacs.model.parameters()])
        out[f'{p}.ema'] = torch.stack([mg.fingerprint(q.data, FP_N) for q in dacs.ema_model.parameters()])
        print(tag, 'iteration', it, {k: round(float(v), 5) for k, v in lv.items()}, 'conf', int(out[f'{p}.pseudo_conf']))
    return dacs


@case
def dacs_step_image():
    out = {'label': image_batch('cs2dsec_image')[0]['label'].to(torch.uint8)}
    _run('dsec', 'cs2dsec_image', 0.0, 3, out)
    dacs = _run('dsec_fd', 'cs2dsec_image', FD_LAMBDA, 3, out)
    keys = list(dacs.state_dict().keys())
    with open(os.path.join(HERE, 'dacs_image_keys.json'), 'w') as f:
        json.dump(keys, f, indent=0)
        f.write('\n')
    print('wrote dacs_image_keys', len(keys), sum(k.startswith('imnet_model.') for k in keys))
    _run('dz', 'cs2dz_image', 0.0, 2, out, with_G=True)
    mg.save('dacs_step_image', **out)


@case
def generator_33():
    G = mg.ns.cyclegan.define_G(input_nc=3, output_nc=3)
    seeded_fill(G, SEEDS['g33'])
    G.eval()
    x = seeded_randn((2, 3, 40, 56), SEEDS['g33'], 'x')
    with torch.no_grad():
        y = G(x)
    mg.save('generator_33', y=y)


@case
def image_simple_test():
    nn.Module.cuda = lambda self, *a, **k: self
    mm = sys.modules['mmseg.models']
    for k in ('BaseSegmentor', 'BaseSegmentorEvents', 'BaseSegmentorFusion'):
        setattr(mm, k, getattr(mg.ns.seg_base, k))
    S = ref_shim.load('mmseg.models.segmentors.encoder_decoder')
    class _Cfg(dict):   # (mmcv's ConfigDict: inference reads test_cfg.mode)
        __getattr__ = dict.__getitem__
    cfg = image_model_cfg()
    cfg.pop('type')
    cfg['test_cfg'] = _Cfg(cfg['test_cfg'])
    m = S.EventsEncoderDecoder(**cfg)
    seeded_fill(m, SEEDS['simple'])
    with torch.no_grad():
        m.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE)
    m.eval()
    img = seeded_randn((1, 3, 440, 640), SEEDS['simple'], 'img')
    out = {}
    with torch.no_grad():
        for key in ('image', 'warp_image'):
            for flip in (False, True):
                meta = dict(ori_shape=(440, 640, 3), flip=flip, flip_direction='horizontal')
                seg = m.simple_test(True, **{key: img, 'img_metas': meta})
                out[f'{key}.flip{int(flip)}'] = np.stack(seg).astype(np.uint8)[..., ::4, ::4]
        logit = m.encode_decode(img, None)
        out['logit_s'] = logit[..., ::16, ::16]
    mg.save('image_simple_test', **out)


if __name__ == '__main__':
    for n in sys.argv[1:] or list(CASES):
        print('==', n)
        CASES[n]()
