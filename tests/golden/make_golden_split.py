"""Generates the fixtures of the split DACS train type 'cs2dz_image+raw-isr_split' from the reference's OWN code (imported unmodified
through ref_shim, with make_golden's helpers and its `dacs_cfg`, the split type set in the model, the head and the uda config):
dacs_step_split.npz -- DACS.train_step (dacs.py:386-395, :481-488, :611-651, :716-771, :797-802; decode_head.py:318-330, :480-507)
for the cases `shared` (share_decoder=True, iterations 0-2 with torch AdamW between them) and `separate` (share_decoder=False,
iteration 0), and FusionEncoderDecoder.simple_test (encoder_decoder.py:897-984) on a 128 x 128 input with ori_shape (96, 160) -- and
dacs_split_keys.json (the DACS state-dict keys).  Runs only in the authoring container.
Usage: python tests/golden/make_golden_split.py [case ...]
"""
import json
import os
import random
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import ref_shim  # noqa: E402
from weights import DACS_SEG_SCALE, dacs_batch, seeded_fill, seeded_randn  # noqa: E402

SPLIT = 'cs2dz_image+raw-isr_split'
SEEDS = dict(student=151, teacher=152, simple=161)
FP_N = 16   # samples per fingerprint
GATES = [(0.13, 0.31, 0.5), (0.07, 0.44, 0.9), (0.18, 0.12, 0.3)]   # (colour-jitter u <= p = 0.2: off, blur u <= 0.5: off, sigma)
CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def split_cfg(share_decoder):
    cfg = mg.dacs_cfg('')
    cfg['train_type'] = cfg['model']['train_type'] = SPLIT
    dp = cfg['model']['decode_head']['decoder_params']
    dp['train_type'], dp['share_decoder'] = SPLIT, share_decoder
    return cfg


def split_batch():
    """dacs_batch's source (image, ISR, label); the target under the Dark Zurich keys `image` / `night_isr` (dacs.py:394-395)"""
    src, tg = dacs_batch()
    return dict(image=src['image'], img_self_res=src['img_self_res'], label=src['label']), dict(image=tg['warp_image'], night_isr=tg['warp_img_self_res'])


def _patch_reference():
    nn.Module.cuda = lambda self, *a, **k: self
    torch.Tensor.cuda = lambda self, *a, **k: self
    mm = sys.modules['mmseg.models']
    for k in ('BaseSegmentor', 'BaseSegmentorEvents', 'BaseSegmentorFusion'):
        setattr(mm, k, getattr(mg.ns.seg_base, k))
    cg = sys.modules['mmseg.models.cyclegan']
    cg.define_G, cg.LightNet = mg.ns.cyclegan.define_G, getattr(mg.ns.cyclegan, 'LightNet', None)


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


def _reference_dacs(share_decoder):
    _patch_reference()
    D = ref_shim.load('mmseg.models.uda.dacs')
    dacs = D.DACS(**split_cfg(share_decoder))
    seeded_fill(dacs.model, SEEDS['student'])
    seeded_fill(dacs.ema_model, SEEDS['teacher'])
    with torch.no_grad():   # peaky classifiers: some pixels of either stream must clear the 0.968 confidence threshold
        dacs.model.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE)
        dacs.model.decode_head.conv_seg_events.weight.mul_(DACS_SEG_SCALE)
    dacs.train()
    D.plt, D.subplotimg = _NoPlot(), (lambda *a, **k: None)
    return dacs


def _run(tag, share_decoder, iters, out):
    dacs = _reference_dacs(share_decoder)
    opt = torch.optim.AdamW(dacs.model.parameters(), lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01)
    src, tg = split_batch()
    model, ema = dacs.get_model(), dacs.get_ema_model()
    captured = {}
    orig_ft, orig_ed = model.forward_train, ema.encode_decode

    def ft(inputs, gt, seg_weight=None, return_feat=False, cfg=None):
        if seg_weight is not None:      # the mixed step (dacs.py:797-802): dict labels, dict weights
            captured.update(mixed_img=inputs['image'].detach().clone(), mixed_isr=inputs['events'].detach().clone(),
                            mixed_lbl={k: v.detach().clone() for k, v in gt.items()},
                            mixed_weight={k: v.detach().clone() for k, v in seg_weight.items()})
        else:
            assert torch.is_tensor(gt), 'the source step passes the plain label to both streams'
        return orig_ft(inputs, gt, seg_weight=seg_weight, return_feat=return_feat, cfg=cfg)

    def ed(*a, **k):
        o = orig_ed(*a, **k)
        assert o.get('fusion_output') is None
        captured['teacher'] = {k: o[k + '_output'].detach().clone() for k in ('image', 'events')}
        return o
    model.forward_train, ema.encode_decode = ft, ed
    uniform = random.uniform
    for it in range(iters):
        seq = iter(GATES[it])
        random.uniform = lambda a, b: next(seq)
        torch.manual_seed(800 + it)
        np.random.seed(800 + it)
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
        names = ['decode.loss_seg', 'decode.acc_seg', 'mix.decode.loss_seg', 'mix.decode.acc_seg']
        p = f'{tag}.it{it}'
        out[f'{p}.losses'] = np.array([lv[k] for k in names])
        out[f'{p}.log_keys'] = np.array(sorted(lv.keys()))
        out[f'{p}.gates'] = np.array(GATES[it])
        out[f'{p}.classes'] = chosen
        plabels, confs = {}, {}
        for s in ('image', 'events'):
            prob, plabels[s] = torch.max(torch.softmax(captured['teacher'][s], dim=1), dim=1)
            confs[s] = int((prob >= 0.968).sum())
            out[f'{p}.{s}.pseudo_label_s'] = plabels[s][..., ::8, ::8].to(torch.uint8)
            out[f'{p}.{s}.pseudo_conf'] = np.array(confs[s])
            out[f'{p}.{s}.teacher_s'] = captured['teacher'][s][..., ::64, ::64]
            out[f'{p}.{s}.mixed_lbl_s'] = captured['mixed_lbl'][s][..., ::8, ::8].to(torch.uint8)
            out[f'{p}.{s}.mixed_weight_s'] = captured['mixed_weight'][s][..., ::8, ::8]
        if it == 0:
            # the streams must be told apart: swapped branches would otherwise pass
            total = plabels['image'].numel()
            assert 0 < confs['image'] < total and 0 < confs['events'] < total and confs['image'] != confs['events'], confs
            differ = (plabels['image'] != plabels['events']).float().mean().item()
            assert differ >= 0.05, f'the two pseudo-labels disagree on {differ:.3%} of the pixels only'
        out[f'{p}.mixed_img_s'] = captured['mixed_img'][..., ::16, ::16]
        out[f'{p}.mixed_isr_s'] = captured['mixed_isr'][:, :1, ::4, ::4].half()
        names = [k for k, _ in dacs.model.named_parameters()]
        assert names == [k for k, _ in dacs.ema_model.named_parameters()]
        out.setdefault(f'{tag}.param_names', np.array(names))
        none = [k for k, q in dacs.model.named_parameters() if q.grad is None]
        out.setdefault(f'{tag}.grad_none', np.array(none))
        assert list(out[f'{tag}.grad_none']) == none and none, none
        zero = lambda q: torch.zeros_like(q) if q.grad is None else q.grad   # noqa: E731  (a row per parameter: zeros where there is none)
        out[f'{p}.grad'] = torch.stack([mg.fingerprint(zero(q), FP_N) for q in dacs.model.parameters()])
        out[f'{p}.ema'] = torch.stack([mg.fingerprint(q.data, FP_N) for q in dacs.ema_model.parameters()])
        print(tag, 'iteration', it, {k: round(float(v), 5) for k, v in lv.items()}, 'conf', confs, 'no gradient:', len(none))
    return dacs


@case
def dacs_step_split():
    out = {}
    dacs = _run('shared', True, 3, out)
    keys = list(dacs.state_dict().keys())
    with open(os.path.join(HERE, 'dacs_split_keys.json'), 'w') as f:
        json.dump(keys, f, indent=0)
        f.write('\n')
    print('wrote dacs_split_keys', len(keys))
    _run('separate', False, 1, out)
    out.update(_simple_test())
    mg.save('dacs_step_split', **out)


def _simple_test():
    _patch_reference()
    S = ref_shim.load('mmseg.models.segmentors.encoder_decoder')

    class _Cfg(dict):   # (mmcv's ConfigDict: inference reads test_cfg.mode)
        __getattr__ = dict.__getitem__
    cfg = split_cfg(True)['model']
    cfg.pop('type')
    cfg['test_cfg'] = _Cfg(cfg['test_cfg'])
    m = S.FusionEncoderDecoder(**cfg)
    seeded_fill(m, SEEDS['simple'])
    with torch.no_grad():
        m.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE)
        m.decode_head.conv_seg_events.weight.mul_(DACS_SEG_SCALE)
    m.eval()
    img = seeded_randn((1, 3, 128, 128), SEEDS['simple'], 'img')
    isr = seeded_randn((1, 3, 128, 128), SEEDS['simple'], 'isr').clamp(-1, 1)
    with torch.no_grad():
        seg = m.simple_test(True, image=img, night_isr=isr, img_metas=dict(ori_shape=(96, 160, 3), flip=False))
        logit = m.encode_decode(img, isr, test_cfg={'output_type': 'events'})
    return {'simple.seg': np.stack(seg).astype(np.uint8), 'simple.logit_s': logit[..., ::8, ::8]}


if __name__ == '__main__':
    for n in sys.argv[1:] or list(CASES):
        print('==', n)
        CASES[n]()
