"""Generates the fixture of the `isr_no_fusion` route of the train type 'cs2dsec_image+events' from the reference's OWN code (imported
unmodified through ref_shim, with make_golden's helpers and its `dacs_cfg`): dacs_step_nofusion.npz -- DACS.train_step (dacs.py:186-195,
:502-523, :667-669, :832-860; encoder_decoder.py:822-823, :833-848) for the cases
  isr      random_choice_thres = 2.0 (every iteration takes the ISR route), lambda_feature_consistency = 0.4 given explicitly,
           iterations 0 and 1 with torch AdamW between them;
  default  the same route, one iteration with the key at -1 (the reference's 0.25);
  events   random_choice_thres = -1.0 (the events route), one iteration: its log keys must NOT contain the consistency term.
Runs only in the authoring container.
Usage: python tests/golden/make_golden_featconsis.py
"""
import os
import random
import sys
import tempfile

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import ref_shim  # noqa: E402
from weights import DACS_SEG_SCALE, dacs_batch, seeded_fill  # noqa: E402

TT = 'cs2dsec_image+events'
SEEDS = dict(student=171, teacher=172, generator=173)
FP_N = 12   # samples per fingerprint
LAMBDA = 0.4
GATES = [(0.13, 0.31, 0.5), (0.07, 0.44, 0.9)]   # (colour-jitter u <= p = 0.2: off, blur u <= 0.5: off, sigma)
CASES = dict(isr=(2.0, LAMBDA, 2), default=(2.0, -1, 1), events=(-1.0, LAMBDA, 1))   # (random_choice_thres, lambda key, iterations)
LOSS_KEYS = ['decode.loss_seg', 'decode.acc_seg', 'decode.loss_feat_consis', 'mix.decode.loss_seg', 'mix.decode.acc_seg',
             'mix.decode.loss_feat_consis', 'loss']


def nofusion_cfg(G_path, lam):
    cfg = mg.dacs_cfg(G_path)
    cfg['train_type'] = cfg['model']['train_type'] = TT
    cfg['model']['decode_head']['decoder_params']['train_type'] = TT
    cfg.update(isr_no_fusion=True, lambda_feature_consistency=lam)
    return cfg


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


def _reference_dacs(thres, lam):
    nn.Module.cuda = lambda self, *a, **k: self
    torch.Tensor.cuda = lambda self, *a, **k: self
    mm = sys.modules['mmseg.models']
    for k in ('BaseSegmentor', 'BaseSegmentorEvents', 'BaseSegmentorFusion'):
        setattr(mm, k, getattr(mg.ns.seg_base, k))
    cg = sys.modules['mmseg.models.cyclegan']
    cg.define_G, cg.LightNet = mg.ns.cyclegan.define_G, getattr(mg.ns.cyclegan, 'LightNet', None)
    D = ref_shim.load('mmseg.models.uda.dacs')
    G = mg.ns.cyclegan.define_G()
    seeded_fill(G, SEEDS['generator'])
    gpath = os.path.join(tempfile.mkdtemp(), 'G.pth')
    torch.save(G.state_dict(), gpath)
    dacs = D.DACS(**nofusion_cfg(gpath, lam))
    dacs.random_choice_thres = thres   # (the constructor only takes the launcher's strings)
    seeded_fill(dacs.model, SEEDS['student'])
    seeded_fill(dacs.ema_model, SEEDS['teacher'])
    with torch.no_grad():
        dacs.model.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE)
    dacs.train()
    D.plt, D.subplotimg = _NoPlot(), (lambda *a, **k: None)
    return dacs


def _run(tag, out):
    thres, lam, iters = CASES[tag]
    dacs = _reference_dacs(thres, lam)
    opt = torch.optim.AdamW(dacs.model.parameters(), lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01)
    src, tg = dacs_batch()
    model, ema = dacs.get_model(), dacs.get_ema_model()
    captured = {}
    orig_ft, orig_ed = model.forward_train, ema.encode_decode

    def ft(inputs, gt, seg_weight=None, return_feat=False, cfg=None):
        step = 'mix' if seg_weight is not None else 'src'
        captured[step + '.no_fusion'] = bool(cfg.get('no_fusion'))
        if step == 'mix':
            captured.update(mixed_img=inputs['image'].detach().clone(), mixed_second=inputs['events'].detach().clone(),
                            mixed_lbl=gt.detach().clone(), mixed_weight=seg_weight.detach().clone())
        return orig_ft(inputs, gt, seg_weight=seg_weight, return_feat=return_feat, cfg=cfg)

    def ed(*a, **k):
        o = orig_ed(*a, **k)
        captured['teacher'] = o['fusion_output'].detach().clone()
        return o
    model.forward_train, ema.encode_decode = ft, ed
    orig_dft = dacs.forward_train

    def dft(**kw):   # train_step drops 'loss' from the log values (dacs.py:304-306): kept here
        lv = orig_dft(**kw)
        captured['loss'] = float(lv['loss'])
        return lv
    dacs.forward_train = dft
    uniform = random.uniform
    for it in range(iters):
        seq = iter(GATES[it])
        random.uniform = lambda a, b: next(seq)
        torch.manual_seed(900 + it)
        np.random.seed(900 + it)
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
        lv = dict(res['log_vars'], loss=captured['loss'])
        p = f'{tag}.it{it}'
        isr_route = tag != 'events'
        assert captured['src.no_fusion'] == captured['mix.no_fusion'] == isr_route
        assert ('decode.loss_feat_consis' in lv) == ('mix.decode.loss_feat_consis' in lv) == isr_route, sorted(lv)
        out[f'{p}.losses'] = np.array([lv.get(k, np.nan) for k in LOSS_KEYS], dtype=np.float64)
        out[f'{p}.log_keys'] = np.array(sorted(res['log_vars'].keys()))
        out[f'{p}.choice'] = float(dacs.forward_cfg['isr_events_fusion_choice'])
        out[f'{p}.gates'] = np.array(GATES[it])
        out[f'{p}.classes'] = chosen
        if isr_route:
            assert abs(lv['loss'] - lv['mix.decode.loss_seg'] - lv['mix.decode.loss_feat_consis']) < 1e-6 * abs(lv['loss'])
        if tag == 'isr':   # the term must not hide inside a gradient tolerance
            for pre in ('', 'mix.'):
                ratio = lv[pre + 'decode.loss_feat_consis'] / lv[pre + 'decode.loss_seg']
                assert ratio >= 0.01, f'{pre}decode.loss_feat_consis is {ratio:.3%} of loss_seg: scale the seeded weights of one encoder'
        prob, plabel = torch.max(torch.softmax(captured['teacher'], dim=1), dim=1)
        conf = int((prob >= 0.968).sum())
        if it == 0:
            assert 0 < conf < plabel.numel(), conf
        out[f'{p}.pseudo_label_s'] = plabel[..., ::8, ::8].to(torch.uint8)
        out[f'{p}.pseudo_conf'] = np.array(conf)
        out[f'{p}.teacher_s'] = captured['teacher'][..., ::64, ::64]
        out[f'{p}.mixed_lbl_s'] = captured['mixed_lbl'][..., ::8, ::8].to(torch.uint8)
        out[f'{p}.mixed_weight_s'] = captured['mixed_weight'][..., ::8, ::8]
        out[f'{p}.mixed_img_s'] = captured['mixed_img'][..., ::16, ::16]
        out[f'{p}.mixed_second_s'] = captured['mixed_second'][:, :1, ::4, ::4].half()
        names = [k for k, _ in dacs.model.named_parameters()]
        assert names == [k for k, _ in dacs.ema_model.named_parameters()]
        out.setdefault('param_names', np.array(names))
        assert list(out['param_names']) == names
        none = [k for k, q in dacs.model.named_parameters() if q.grad is None]
        out[f'{tag}.grad_none'] = np.array(none)
        zero = lambda q: torch.zeros_like(q) if q.grad is None else q.grad   # noqa: E731  (a row per parameter: zeros where there is none)
        out[f'{p}.grad'] = torch.stack([mg.fingerprint(zero(q), FP_N) for q in dacs.model.parameters()])
        out[f'{p}.ema'] = torch.stack([mg.fingerprint(q.data, FP_N) for q in dacs.ema_model.parameters()])
        print(tag, 'iteration', it, {k: round(float(v), 6) for k, v in lv.items()}, 'conf', conf, 'no gradient:', len(none))


if __name__ == '__main__':
    out = {'lambda': np.array(LAMBDA)}
    for tag in sys.argv[1:] or list(CASES):
        print('==', tag)
        _run(tag, out)
    if not sys.argv[1:]:
        mg.save('dacs_step_nofusion', **out)
