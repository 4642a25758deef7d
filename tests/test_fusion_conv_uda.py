"""One DACS iteration with the convolutional fusion modules (ConvertAvgFusion, AverageFusion) against oracle/dacs_iter.py run on oracle
segmentors whose fusion module is a plain-torch module written out here (mmseg/models/fusion/convert_avg_fusion.py, average_fusion.py,
backbones/resnet.py:15-100 restated).  Reduced widths (test_dacs.SMALL), fp32, B = 2, 64 x 64, with the source and the mixed step as
ONE student pass (per-pass BatchNorm statistics: segmentors._extract_joint hands the pass count to the module) and as two passes.
Bounds: test_dacs.check_iteration's (1e-4, 5e-2) and run_case's running-statistic bounds."""
import os
import random
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
from weights import seeded_fill  # noqa: E402

import cmda_amd  # noqa: E402,F401
import cmda_amd.runtime as rt  # noqa: E402
from cmda_amd.registry import build_train_model  # noqa: E402
from conftest import assert_close  # noqa: E402
from oracle import cyclegan as ocg, dacs_iter, head as ohd, mit as omit, segmentor as oseg  # noqa: E402
from test_dacs import DEPTHS, FCFG, FULLW, ISR, SMALL, check_iteration, make_batch, make_cfg, oracle_draws  # noqa: E402


class TorchBasicBlock(nn.Module):
    def __init__(self, planes):
        super().__init__()
        self.conv1 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)

    def forward(self, x):
        return torch.relu(self.bn2(self.conv2(torch.relu(self.bn1(self.conv1(x))))) + x)


class TorchConvertAvgFusion(nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.basic_block = nn.ModuleList([TorchBasicBlock(dims[i // 2]) for i in range(8)])

    def forward(self, image_features, events_features):
        return [(self.basic_block[2 * i](a) + self.basic_block[2 * i + 1](b)) / 2 for i, (a, b) in enumerate(zip(image_features, events_features))]


class TorchAverageFusion(nn.Module):
    def forward(self, image_features, events_features):
        return [(a + b) / 2 for a, b in zip(image_features, events_features)]


def fusion_cfg(name, dims):
    return dict(type=name, in_channels=dims, out_channels=dims) if name == 'ConvertAvgFusion' else dict(type=name)


def torch_fusion(name, dims):
    return TorchConvertAvgFusion(dims) if name == 'ConvertAvgFusion' else TorchAverageFusion()


def oracle_student(dims, ch, fusion, fusion_isr=None):
    return oseg.FusionEncoderDecoder(backbone_image=omit.MixVisionTransformer(embed_dims=dims, depths=DEPTHS, drop_path_rate=0.0),
                                     backbone_events=omit.MixVisionTransformer(embed_dims=dims, depths=DEPTHS, drop_path_rate=0.0),
                                     fusion_module=torch_fusion(fusion, dims),
                                     fusion_isr_module=torch_fusion(fusion_isr, dims) if fusion_isr else None,
                                     decode_head=ohd.DAFormerHeadFusion(in_channels=dims, channels=ch, embed_dims=ch, dropout_ratio=0.0,
                                                                        share_decoder=True))


def build(tgt, dims, ch, dtype, fusion, fused, fusion_isr=None):
    rt.set_compute_dtype(dtype)
    cfg = make_cfg(dims, ch)
    cfg['model']['fusion_module'] = fusion_cfg(fusion, dims)
    if fusion_isr:
        cfg['model']['fusion_isr_module'] = fusion_cfg(fusion_isr, dims)
        cfg['uda']['isr_another_fusion'] = True
    dacs = build_train_model(cfg)
    seeded_fill(dacs.model, 7)
    seeded_fill(dacs.ema_model, 8)
    seeded_fill(dacs.cyclegan_itrd2en, 9)
    dacs.to(tgt.device).train()
    dacs.fused_student_passes = fused
    if fusion_isr:
        dacs.random_choice_thres = 2.0   # never the events: every pass takes the ISR route through fusion_isr_module
    return dacs


def run(tgt, fusion, fused, fusion_isr=None):
    dims, ch = SMALL['dims'], SMALL['ch']
    dacs = build(tgt, dims, ch, torch.float32, fusion, fused, fusion_isr)
    src, tg = make_batch(2, 64, 64)
    batch = dict(source={k: tgt.to(v) for k, v in src.items()}, target={k: tgt.to(v) for k, v in tg.items()})
    ref, ema, G = oracle_student(dims, ch, fusion, fusion_isr), oracle_student(dims, ch, fusion, fusion_isr), ocg.ResnetGenerator().eval()
    seeded_fill(ref, 7).train()
    seeded_fill(ema, 8).train()
    seeded_fill(G, 9)
    torch.manual_seed(11), random.seed(11), np.random.seed(11)
    log_vars = dacs(**batch)
    mix = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in dacs.last_mix.items()}
    zero = lambda p: torch.zeros_like(p.detach().cpu())
    grads = {n: (p.grad.detach().cpu().clone() if p.grad is not None else zero(p)) for n, p in dacs.model.named_parameters()}
    fcfg = dict(FCFG, fusion_isr=True) if fusion_isr else FCFG
    o = dacs_iter.dacs_iteration(ref, ema, G, src, tg, local_iter=0, forward_cfg=fcfg, isr_parms=ISR, shift_type='random',
                                 draws=oracle_draws(dacs.last_draws), random_choice_thres=2.0 if fusion_isr else 0.5)
    assert o['use_events'] == (not fusion_isr and dacs.last_draws['choice'] > 0.5)
    ref_grads = {n: (q.grad.clone() if q.grad is not None else zero(q)) for n, q in ref.named_parameters()}
    check_iteration(({k: v.detach().clone() for k, v in log_vars.items()}, mix, grads, o, ref_grads), True, 1e-4, 5e-2)
    # BatchNorm running statistics, the fusion modules' included: the student's after the source and the mixed step (in that order), the
    # teacher's after its one train-mode pass
    for who, mine, theirs in (('student', dacs.model, ref), ('teacher', dacs.ema_model, ema)):
        mine = dict(mine.named_buffers())
        seen = fus = 0
        for n, b in theirs.named_buffers():
            if 'running_' in n:
                assert_close(mine[n], b, 1e-4, atol=1e-5, name=f'{who} {n}')
                seen += 1
                fus += n.startswith(('fusion_module.', 'fusion_isr_module.'))
        assert seen > 0 and fus == 32 * ((fusion == 'ConvertAvgFusion') + (fusion_isr == 'ConvertAvgFusion'))
    return dacs


@pytest.mark.parametrize('fused', [True, False], ids=['one_pass', 'two_passes'])
@pytest.mark.parametrize('fusion', ['ConvertAvgFusion', 'AverageFusion'])
def test_dacs_iteration_with_convolutional_fusion(tgt, fusion, fused):
    try:
        dacs = run(tgt, fusion, fused)
        assert dacs.fused_student_passes == fused
    finally:
        rt.set_compute_dtype(torch.float32)


def test_dacs_iteration_with_convolutional_isr_fusion(tgt):
    """fusion_isr_module=dict(type='ConvertAvgFusion') with isr_another_fusion: the ISR route (image + ISR through the second fusion
    module) in the student's two passes and in the teacher, through the same fwd / bwd pair"""
    try:
        run(tgt, 'ConvertAvgFusion', True, fusion_isr='ConvertAvgFusion')
    finally:
        rt.set_compute_dtype(torch.float32)


@pytest.mark.gpu
def test_dacs_captured_iteration_with_convolutional_fusion_gpu():
    """bf16, MiT-B5 widths, the iteration captured as a hipGraph (one eager warm-up iteration, one captured and replayed): every loss
    finite"""
    from conftest import Target
    from cmda_amd import _lib
    _lib._unbind_for_tests()
    if not torch.cuda.is_available():
        pytest.skip('no GPU on this machine')
    tgt = Target('gpu')
    try:
        dacs = build(tgt, FULLW['dims'], FULLW['ch'], torch.bfloat16, 'ConvertAvgFusion', True)
        src, tg = make_batch(2, 128, 128)
        batch = dict(source={k: tgt.to(v) for k, v in src.items()}, target={k: tgt.to(v) for k, v in tg.items()})
        torch.manual_seed(11), random.seed(11), np.random.seed(11)
        dacs.enable_graph(warmup_iters=1)
        for it in range(2):
            log_vars = dacs(**batch)
            for k in ('decode.loss_seg', 'mix.decode.loss_seg'):
                assert torch.isfinite(log_vars[k]).all().item(), f'iteration {it}: {k} = {log_vars[k]}'
        assert dacs._graph is not None, 'the iteration was not captured'
        torch.cuda.synchronize()
        for n, b in dacs.model.named_buffers():
            if 'running_' in n and n.startswith('fusion_module.'):
                assert torch.isfinite(b).all().item(), n
    finally:
        rt.set_compute_dtype(torch.float32)
