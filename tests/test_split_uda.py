"""The split DACS train type 'cs2dz_image+raw-isr_split' (two streams, no fusion block; dacs.py:611-651, :716-771, :797-802;
decode_head.py:318-330, :480-507, :563-586; encoder_decoder.py:903-904, :919-920): construction and state-dict keys, the refusals,
the decode head's split classifiers and dict targets, the optimiser leaving never-read parameters alone, the inference rule, one
small iteration on the emulator and the GPU, and on the GPU the whole step against the reference's own code
(tests/golden/dacs_step_split.npz, dacs_split_keys.json, written by tests/golden/make_golden_split.py), graph replay against eager
and simple_test."""
import json
import os
import random
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
from weights import DACS_CH, DACS_DIMS, DACS_SEG_SCALE, dacs_batch, sample_grad, seeded_fill, seeded_randn  # noqa: E402

import cmda_amd  # noqa: E402,F401
import cmda_amd.runtime as rt  # noqa: E402
import test_dacs as TD  # noqa: E402
from cmda_amd import ops  # noqa: E402
from cmda_amd.registry import build_segmentor, build_train_model  # noqa: E402
from conftest import assert_close, check_le  # noqa: E402

SPLIT = 'cs2dz_image+raw-isr_split'
SEEDS = dict(student=151, teacher=152, simple=161)   # make_golden_split.SEEDS
FP_N = 16
DIRECT = [['leftdown', 'leftup'], ['rightdown', 'rightup']]
FCFG = dict(loss_weight={'image': 0.5, 'events': 0.5, 'fusion': 0.5, 'img_self_res': 0.25}, gradual_rate=0.0)


def golden(name):
    return {k: (v.tolist() if v.dtype.kind == 'U' else torch.from_numpy(v)) for k, v in np.load(os.path.join(HERE, 'golden', name)).items()}


def make_cfg(dims=DACS_DIMS, ch=DACS_CH, share_decoder=True, train_type=SPLIT, **uda):
    """the reference's config keys of the fusion fixtures (make_golden.dacs_cfg) with the train type set in the model, the head and
    the uda section, as make_golden_split.split_cfg does"""
    cfg = TD.make_cfg(dims, ch, generator=False, train_type=train_type)
    cfg['model']['decode_head']['decoder_params']['share_decoder'] = share_decoder
    cfg['uda'].update(uda)
    return cfg


def split_batch():
    """make_golden_split.split_batch"""
    src, tg = dacs_batch()
    return dict(image=src['image'], img_self_res=src['img_self_res'], label=src['label']), dict(image=tg['warp_image'], night_isr=tg['warp_img_self_res'])


def small_batch(B=2, H=64, W=64):
    src, tg = TD.make_batch(B, H, W)
    return dict(image=src['image'], img_self_res=src['img_self_res'], label=src['label']), dict(image=tg['warp_image'], night_isr=tg['warp_img_self_res'])


# ---------------------------------------------------------------------------------------------------------------------------
# construction (no GPU)
@pytest.mark.parametrize('share', [True, False])
def test_split_builds_from_reference_config_keys(share):
    with torch.device('meta'):
        dacs = build_train_model(make_cfg(share_decoder=share))
    assert dacs.train_type == SPLIT and dacs.model.fusion_module is None and dacs.model.decode_head.split_cls
    assert not dacs.model.decode_head.joint_ok(), 'the joint decoder pass is not extended to two classifiers'
    keys = list(dacs.state_dict().keys())
    for k in ('conv_seg_events.weight', 'conv_seg_events.bias', 'conv_seg_fusion.weight', 'conv_seg_fusion.bias'):
        assert f'model.decode_head.{k}' in keys and f'ema_model.decode_head.{k}' in keys
    unread = sorted(n for n, p in dacs.model.named_parameters() if getattr(p, '_cmda_unread', False))
    if share:
        assert sorted(keys) == sorted(json.load(open(os.path.join(HERE, 'golden', 'dacs_split_keys.json'))))
        assert unread == ['decode_head.conv_seg_fusion.bias', 'decode_head.conv_seg_fusion.weight']
    else:
        assert all(n.startswith(('decode_head.conv_seg_fusion.', 'decode_head.embed_layers_fusion.', 'decode_head.fuse_layer_fusion.'))
                   for n in unread)
        assert any(n.startswith('decode_head.fuse_layer_fusion.') for n in unread)
    g = golden('dacs_step_split.npz')
    assert unread == sorted(g['shared.grad_none' if share else 'separate.grad_none']), 'what the reference leaves without a gradient'


def test_split_with_feature_distance_is_refused():
    with pytest.raises(ValueError, match=r'feature.distance.*dacs\.py:568-575'):
        with torch.device('meta'):
            build_train_model(make_cfg(imnet_feature_dist_lambda=0.005))


def test_no_fusion_and_d2n_isr_are_still_refused():
    with pytest.raises(ValueError, match=r'dacs\.py:809.*encoder_decoder\.py:703'):
        with torch.device('meta'):
            build_train_model(make_cfg(train_type='cs2dz_image+raw-isr_no-fusion'))
    with pytest.raises(ValueError, match='pre-translated ISR'):
        with torch.device('meta'):
            build_train_model(make_cfg(train_type='cs2dz_image+d2n-isr'))
    from cmda_amd import decode_heads as dh
    with pytest.raises(AssertionError, match=r'dacs\.py:809'):
        dh.DAFormerHeadFusion(**HEAD_KW, decoder_params=decoder_params(train_type='cs2dz_image+raw-isr_no-fusion'))


def test_split_draw_has_no_events_choice():
    with torch.device('meta'):
        dacs = build_train_model(make_cfg())
    lab = torch.randint(0, 19, (2, 1, 16, 16), generator=torch.Generator().manual_seed(0))
    torch.manual_seed(5)
    before = torch.rand(1)
    torch.manual_seed(5)
    d = dacs._draw(lab, 16, 16)
    assert d['choice'] == 0.0 and torch.equal(torch.rand(1), before), 'no torch.rand: dacs.py:414-417 is in the events branch only'


# ---------------------------------------------------------------------------------------------------------------------------
# decode head (emulator and GPU)
HEAD_KW = dict(in_channels=[32, 64, 160, 256], in_index=[0, 1, 2, 3], channels=64, dropout_ratio=0.0, num_classes=19,
               norm_cfg=dict(type='BN', requires_grad=True), align_corners=False,
               loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))


def decoder_params(**extra):
    d = dict(embed_dims=64, embed_cfg=dict(type='mlp', act_cfg=None, norm_cfg=None), embed_neck_cfg=dict(type='mlp', act_cfg=None, norm_cfg=None),
             fusion_cfg=dict(type='aspp', sep=True, dilations=(1, 6, 12, 18), pool=False, act_cfg=dict(type='ReLU'),
                             norm_cfg=dict(type='BN', requires_grad=True)))
    d.update(extra)
    return d


def feats_nlc(tgt, B, H, W, seed, tag):
    out = []
    for i, (c, s) in enumerate(zip(HEAD_KW['in_channels'], [4, 8, 16, 32])):
        h, w = max(H // s, 1), max(W // s, 1)
        f = seeded_randn((B, c, h, w), seed, f'{tag}{i}')
        out.append((tgt.to(f.permute(0, 2, 3, 1).reshape(-1, c).contiguous()), h, w))
    return out


def split_head(tgt, share=True, **kw):
    from cmda_amd import decode_heads as dh
    rt.set_compute_dtype(torch.float32)
    head = dh.DAFormerHeadFusion(**dict(HEAD_KW, **kw), decoder_params=decoder_params(train_type=SPLIT, share_decoder=share))
    seeded_fill(head, 51)
    with torch.no_grad():
        head.conv_seg.weight.mul_(DACS_SEG_SCALE), head.conv_seg_events.weight.mul_(DACS_SEG_SCALE)
    return head.train().to(tgt.device)


def head_targets(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    gts, wts = {}, {}
    for k in ('image', 'events'):
        gt = torch.randint(0, 19, (B, 1, H, W), generator=g)
        gt[torch.rand(B, 1, H, W, generator=g) < 0.1] = 255
        gts[k], wts[k] = gt, torch.rand(B, H, W, generator=g)
    return gts, wts


def test_head_dict_targets_of_one_tensor_equal_the_plain_tensor(tgt):
    """the same logits through the loss mix with plain targets and with dicts holding those targets twice: loss, accuracy and the
    logit gradients bit for bit.  The labels cover one 64 x 8 tile per sample and there is one sample, so that each cross-entropy
    sum is one workgroup's (the kernel adds one partial per workgroup with a float atomic: over several the order is free)."""
    from cmda_amd import decode_heads as dh
    head = split_head(tgt)
    B, H, W = 1, 8, 64
    inputs = {'f_image': feats_nlc(tgt, B, 32, 256, 52, 'i'), 'f_events': feats_nlc(tgt, B, 32, 256, 52, 'e')}
    gts, wts = head_targets(B, H, W, 53)
    gt, wt = tgt.to(gts['image']), tgt.to(wts['image'])
    logits, _ = head.fwd(inputs, B)
    assert logits['fusion_output'] is None and logits['img_self_res_output'] is None
    for weight in (wt, None):
        plain, sv_p, coef_p = head._loss_mix(logits, gt, weight, FCFG)
        dicts, sv_d, coef_d = head._loss_mix(logits, {'image': gt, 'events': gt},
                                             None if weight is None else {'image': weight, 'events': weight}, FCFG)
        assert coef_p == coef_d == {'image_output': 1.0, 'events_output': 1.0}
        assert torch.equal(plain['loss_seg'].cpu(), dicts['loss_seg'].cpu()) and torch.equal(plain['acc_seg'].cpu(), dicts['acc_seg'].cpu())
        for k in ('image_output', 'events_output'):
            dp = dh.ce_losses_bwd(sv_p[k], None, coef_p[k], head.ignore_index, 1.0)
            dd = dh.ce_losses_bwd(sv_d[k], None, coef_d[k], head.ignore_index, 1.0)
            assert torch.equal(dp.cpu(), dd.cpu()) and bool(dp.abs().sum().item() > 0), k
    # and through fwd_train: the same entry point the segmentor calls
    losses, _, _ = head.fwd_train(inputs, B, {'image': gt, 'events': gt}, {'image': wt, 'events': wt}, FCFG)
    ref, _, _ = head.fwd_train(inputs, B, gt, wt, FCFG)
    assert_close(losses['loss_seg'], ref['loss_seg'], 1e-5, name='fwd_train, dict of one tensor against the tensor')


def _restated_loss(logit_nhwc, gt, weight):
    """decode_head.py:588-606 in float64: resize, cross-entropy (ignore 255, reduction none) * weight, mean over ALL pixels; accuracy"""
    up = F.interpolate(logit_nhwc.permute(0, 3, 1, 2).double().cpu(), size=gt.shape[2:], mode='bilinear', align_corners=False)
    ce = F.cross_entropy(up, gt[:, 0], reduction='none', ignore_index=255)
    acc = (up.argmax(1) == gt[:, 0]).double().mean() * 100
    return (ce * weight.double()).mean(), acc


def test_head_distinct_dict_targets_match_float64_restatement(tgt):
    """decode_head.py:501-507 restated in float64 on the head's own logits; the bound is test_modules.py's for the head's loss (1e-5)"""
    head = split_head(tgt)
    B, H, W = 2, 40, 72   # logits 10 x 18: several tiles per sample, a partial one at the right and at the bottom
    inputs = {'f_image': feats_nlc(tgt, B, H, W, 54, 'i'), 'f_events': feats_nlc(tgt, B, H, W, 54, 'e')}
    gts, wts = head_targets(B, H, W, 55)
    losses, logits, saved = head.fwd_train(inputs, B, {k: tgt.to(v) for k, v in gts.items()}, {k: tgt.to(v) for k, v in wts.items()}, FCFG)
    li, acc_i = _restated_loss(logits['image_output'], gts['image'], wts['image'])
    le, _ = _restated_loss(logits['events_output'], gts['events'], wts['events'])
    ref = li * 0.5 * 2 + le * 0.5 * 2
    assert abs(float(li) - float(le)) > 1e-2 * float(ref), 'the two terms differ: swapped targets would show'
    assert_close(losses['loss_seg'], ref.float(), 1e-5, name='split loss')
    assert_close(losses['acc_seg'], acc_i.float().view(1), 1e-6, name='accuracy: the image branch\'s')
    # a None weight means ones
    losses1, logits1, _ = head.fwd_train(inputs, B, {k: tgt.to(v) for k, v in gts.items()}, None, FCFG)
    ones = torch.ones(B, H, W)
    ref1 = _restated_loss(logits1['image_output'], gts['image'], ones)[0] * 0.5 * 2 + _restated_loss(logits1['events_output'], gts['events'], ones)[0] * 0.5 * 2
    assert_close(losses1['loss_seg'], ref1.float(), 1e-5, name='split loss, no weight')


@pytest.mark.parametrize('share', [True, False])
def test_head_branch_gradients_reach_their_own_classifier(tgt, share):
    head = split_head(tgt, share)
    B, H, W = 1, 32, 32
    inputs = {'f_image': feats_nlc(tgt, B, H, W, 56, 'i'), 'f_events': feats_nlc(tgt, B, H, W, 56, 'e')}
    logits, saved = head.fwd(inputs, B)
    dl = tgt.to(seeded_randn(logits['events_output'].shape, 57, 'dl'))
    dfs = head.bwd(saved, {'events_output': dl, 'image_output': None}, B)
    ops.gemm_flush_deferred()
    nz = lambda p: p.grad is not None and bool(p.grad.abs().sum().item() > 0)   # noqa: E731
    assert set(dfs) == {'f_events'}
    assert nz(head.conv_seg_events.weight) and nz(head.conv_seg_events.bias)
    assert not nz(head.conv_seg.weight) and not nz(head.conv_seg.bias), 'the events branch reached the image classifier'
    assert not nz(head.conv_seg_fusion.weight) and not nz(head.conv_seg_fusion.bias)
    for p in head.parameters():
        p.grad = None
    dfs = head.bwd(saved, {'image_output': dl, 'events_output': None}, B)
    ops.gemm_flush_deferred()
    assert set(dfs) == {'f_image'} and nz(head.conv_seg.weight) and not nz(head.conv_seg_events.weight)
    for n, p in head.named_parameters():
        if getattr(p, '_cmda_unread', False):
            assert not nz(p), f'{n} is never read'


def test_head_loss_weight_assert(tgt):
    head = split_head(tgt)
    B, H, W = 1, 32, 32
    inputs = {'f_image': feats_nlc(tgt, B, H, W, 58, 'i'), 'f_events': feats_nlc(tgt, B, H, W, 58, 'e')}
    gt = tgt.to(head_targets(B, H, W, 59)[0]['image'])
    for lw in ({'image': 0.5, 'events': 0.25}, {'image': 1.0, 'events': 0.5}):
        with pytest.raises(AssertionError, match='0.5'):
            head.fwd_train(inputs, B, gt, None, dict(loss_weight=dict(FCFG['loss_weight'], **lw)))


def test_head_events_dropout_takes_its_own_draw_after_the_image_branch(tgt):
    head = split_head(tgt, dropout_ratio=0.5)
    B, H, W = 2, 32, 32
    inputs = {'f_image': feats_nlc(tgt, B, H, W, 60, 'i'), 'f_events': feats_nlc(tgt, B, H, W, 60, 'e')}
    rt.taps = {}
    try:
        torch.manual_seed(3)
        head.fwd(inputs, B)
        taps = {k[1]: v.cpu() for k, v in rt.taps.items() if k[0] == 'dropout2d'}
    finally:
        rt.taps = None
    assert sorted(taps) == ['DAFormerHeadFusion', 'DAFormerHeadFusion_events']
    torch.manual_seed(3)
    first = (torch.rand(B, 64, device=tgt.device) < 0.5).float().cpu()
    second = (torch.rand(B, 64, device=tgt.device) < 0.5).float().cpu()
    assert torch.equal(taps['DAFormerHeadFusion'], first) and torch.equal(taps['DAFormerHeadFusion_events'], second)
    # an injected mask drives the events branch's Dropout2d: all channels dropped -> the logits are the classifier's bias
    head.inject_dropout_mask_events = torch.zeros(B, 64)
    logits, _ = head.fwd(inputs, B)
    bias = head.conv_seg_events.bias.detach().cpu().view(1, 1, 1, -1).expand_as(logits['events_output'])
    assert_close(logits['events_output'], bias, 1e-6, name='events logits with every channel dropped')


# ---------------------------------------------------------------------------------------------------------------------------
# optimiser: never-read parameters
def test_flat_adamw_leaves_never_read_parameters_alone(tgt):
    from cmda_amd.optim import FlatAdamW
    head = split_head(tgt, share=False)
    init = {n: p.detach().cpu().clone() for n, p in head.named_parameters()}
    unread = [n for n, p in head.named_parameters() if getattr(p, '_cmda_unread', False)]
    assert 'conv_seg_fusion.weight' in unread and any(n.startswith('fuse_layer_fusion.') for n in unread)
    opt = FlatAdamW(head, lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01, custom_keys=dict(head=dict(lr_mult=10.0)))
    assert opt.unread_range is not None and all(e <= opt.unread_range[0] for _, e, _, _ in opt.segments)
    for n, p in head.named_parameters():
        assert torch.equal(p.detach().cpu(), init[n]), f'{n} moved into the flat store unchanged'
    for _ in range(3):
        opt.zero_grad()
        opt.flat_g[:opt.unread_range[0]].normal_(generator=None)
        opt.step()
    for n, p in head.named_parameters():
        same = torch.equal(p.detach().cpu(), init[n])
        assert same == (n in unread), f'{n}: {"changed" if not same else "unchanged"} after three steps'
    sd = opt.state_dict()
    order = [n for n, _ in head.named_parameters()]
    assert len(sd['param_groups']) == len(order)
    assert sorted(sd['state']) == [i for i, n in enumerate(order) if n not in unread], 'no state for a parameter without a gradient'
    opt.load_state_dict(sd)
    assert opt.step_count == 3
    assert set(head.state_dict()) >= {'conv_seg_fusion.weight', 'conv_seg_fusion.bias'}


# ---------------------------------------------------------------------------------------------------------------------------
# inference (emulator and GPU)
def split_segmentor(tgt, test_cfg=None, dims=(32, 64, 160, 256), ch=64, seed=61):
    rt.set_compute_dtype(torch.float32)
    cfg = make_cfg(list(dims), ch)['model']
    if test_cfg is not None:
        cfg['test_cfg'] = test_cfg
    m = build_segmentor(cfg)
    seeded_fill(m, seed)
    with torch.no_grad():
        m.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE), m.decode_head.conv_seg_events.weight.mul_(DACS_SEG_SCALE)
    return m.to(tgt.device).eval()


def test_split_predict_is_the_argmax_of_the_events_output(tgt):
    m = split_segmentor(tgt)
    img, isr = tgt.to(seeded_randn((1, 3, 64, 96), 62, 'img')), tgt.to(seeded_randn((1, 3, 64, 96), 62, 'isr').clamp(-1, 1))
    both = m.encode_decode(img, isr, output_features=True)   # the two-stream pass (the teacher's)
    assert both['fusion_output'] is None and both['image_output'] is not None and both['events_output'].shape == (1, 19, 64, 96)
    assert not torch.equal(both['image_output'].argmax(1).cpu(), both['events_output'].argmax(1).cpu())
    calls = []
    orig = m.backbone_image.fwd
    m.backbone_image.fwd = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    lab = m.predict(False, image=img, night_isr=isr, img_metas=dict(ori_shape=(64, 96, 3), flip=False))
    assert lab.dtype == torch.uint8 and torch.equal(lab.cpu().long(), both['events_output'].argmax(1).cpu())
    seg = m.simple_test(False, image=img, night_isr=isr, img_metas=dict(ori_shape=(64, 96, 3), flip=False))
    assert np.array_equal(np.stack(seg), both['events_output'].argmax(1).cpu().numpy())
    aug = m.predict_aug([dict(image=img, night_isr=isr, img_metas=dict(ori_shape=(64, 96, 3), flip=False))])
    assert torch.equal(aug.cpu().long(), torch.softmax(both['events_output'], 1).argmax(1).cpu())
    assert not calls, 'the image encoder ran at test time'


def test_split_inference_needs_night_isr(tgt):
    m = split_segmentor(tgt)
    img = tgt.to(seeded_randn((1, 3, 64, 64), 62, 'img'))
    for call in (lambda: m.predict(False, image=img), lambda: m.simple_test(False, image=img, img_metas=dict(ori_shape=(64, 64, 3))),
                 lambda: m.predict_aug([dict(image=img, img_metas=dict(ori_shape=(64, 64, 3)))]),
                 lambda: m.slide_inference(False, image=img)):
        with pytest.raises(KeyError, match='night_isr'):
            call()


def test_split_slide_mode_crops_night_isr_with_the_image(tgt):
    m = split_segmentor(tgt, test_cfg=dict(mode='slide', crop_size=(64, 64), stride=(32, 32)))
    img, isr = tgt.to(seeded_randn((1, 3, 96, 96), 63, 'img')), tgt.to(seeded_randn((1, 3, 96, 96), 63, 'isr').clamp(-1, 1))
    seen = []
    orig = m.encode_decode_lowres

    def spy(image, events, *a, **k):
        seen.append((image, events.cpu()))
        return orig(image, events, *a, **k)
    m.encode_decode_lowres = spy
    meta = dict(ori_shape=(96, 96, 3), flip=False)
    lab = m.predict(True, image=img, night_isr=isr, img_metas=meta)
    wins = ops.slide_windows(96, 96, (64, 64), (32, 32))
    assert len(wins) == 4 and len(seen) == 1 and seen[0][0] is None
    assert torch.equal(seen[0][1], torch.cat([isr.cpu()[:, :, y1:y2, x1:x2] for y1, x1, y2, x2 in wins]))
    m.encode_decode_lowres = orig
    ref = m.slide_inference(True, image=img, night_isr=isr, img_metas=meta).argmax(1)
    check_le('slide predict vs slide_inference: label disagreement', (lab.cpu().long() != ref.cpu()).float().mean().item(), 1e-3)


# ---------------------------------------------------------------------------------------------------------------------------
# one small iteration (emulator and GPU)
def test_split_targets_pair_and_composed_sequence_agree(tgt):
    """DACS._split_targets both ways (`split_fused_targets`): the kernel pair and `_mix_targets` per stream give the same tensors"""
    with torch.device('meta'):
        dacs = build_train_model(make_cfg([32, 64, 160, 256], 64, pseudo_weight_ignore_top=3, pseudo_weight_ignore_bottom=5))
    B, H, W = 2, 40, 72
    g = torch.Generator().manual_seed(71)
    lg = [tgt.to(torch.randn(B, 10, 18, 19, generator=g) * s) for s in (8.0, 16.0)]
    lab = tgt.to(torch.randint(0, 6, (B, H // 8, W // 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous())
    classes = tgt.to(torch.tensor([[0, 3, 5] + [-1] * 7, [1, 2, -1] + [-1] * 7]))
    outs = []
    for fused in (True, False):
        dacs.split_fused_targets = fused
        outs.append(dacs._split_targets(lg[0], lg[1], lab, classes))
    (p0, c0, m0, w0), (p1, c1, m1, w1) = outs
    assert torch.equal(p0.cpu(), p1.cpu()) and torch.equal(c0.cpu(), c1.cpu()) and int(c0[0]) != int(c0[1])
    for k in ('image', 'events'):
        assert m0[k].shape == (B, 1, H, W) and w0[k].shape == (B, H, W)
        assert torch.equal(m0[k].cpu(), m1[k].cpu()) and torch.equal(w0[k].cpu(), w1[k].cpu())
    assert not torch.equal(m0['image'].cpu(), m0['events'].cpu())


def test_split_iteration_targets_and_gradients(tgt):
    rt.set_compute_dtype(torch.float32)
    dacs = build_train_model(make_cfg([32, 64, 160, 256], 64, pseudo_weight_ignore_top=3, pseudo_weight_ignore_bottom=5))
    seeded_fill(dacs.model, 7)
    seeded_fill(dacs.ema_model, 8)
    with torch.no_grad():
        dacs.model.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE), dacs.model.decode_head.conv_seg_events.weight.mul_(DACS_SEG_SCALE)
    dacs.to(tgt.device).train()
    src, tg = small_batch(B=1)
    B, H, W = 1, 64, 64
    torch.manual_seed(11), random.seed(11), np.random.seed(11)
    lv = dacs(source={k: tgt.to(v) for k, v in src.items()}, target={k: tgt.to(v) for k, v in tg.items()})
    assert sorted(lv) == ['decode.acc_seg', 'decode.loss_seg', 'loss', 'mix.decode.acc_seg', 'mix.decode.loss_seg']
    assert all(np.isfinite(float(v)) for v in lv.values())
    mix = dacs.last_mix
    ema, lab, classes = mix['teacher_logits'], tgt.to(src['label']).view(B, H, W), mix['classes']
    assert ema['fusion_output'] is None
    for s, suffix in (('image', ''), ('events', '_events')):
        pseudo, _, count = ops.pseudo_label(ema[s + '_output'], H, W, 0.968, want_prob=False)
        pw = ops.pseudo_weight(count, B, H, W, 3, 5)
        mixed = ops.class_mix_label(lab, pseudo, lab, classes)
        weight = ops.class_mix(torch.ones_like(pw).view(B, 1, H, W), pw.view(B, 1, H, W), lab, classes).view(B, H, W)
        assert torch.equal(mix['pseudo_label' + suffix].cpu(), pseudo.cpu()) and int(mix['pseudo_count' + suffix]) == int(count)
        assert torch.equal(mix['mixed_lbl' + suffix].cpu().view(B, H, W), mixed.cpu()), s
        assert torch.equal(mix['pseudo_weight' + suffix].cpu(), weight.cpu()), s
    assert not torch.equal(mix['pseudo_label'].cpu(), mix['pseudo_label_events'].cpu())
    head = dacs.model.decode_head
    assert head.conv_seg_fusion.weight.grad is None, 'never read: no gradient'
    for conv in (head.conv_seg, head.conv_seg_events):
        assert conv.weight.grad is not None and bool(conv.weight.grad.abs().sum().item() > 0)
    for bb in (dacs.model.backbone_image, dacs.model.backbone_events):
        assert all(p.grad is not None for p in bb.parameters())


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
def _gpu():
    from conftest import Target
    from cmda_amd import _lib
    _lib._unbind_for_tests()
    if not torch.cuda.is_available():
        pytest.skip('no GPU on this machine')
    return Target('gpu')


@pytest.mark.gpu
def test_split_simple_test_against_reference_gpu():
    """the bounds of test_image_uda.py::test_simple_test_against_reference_gpu"""
    tgt = _gpu()
    g = golden('dacs_step_split.npz')
    m = split_segmentor(tgt, dims=DACS_DIMS, ch=DACS_CH, seed=SEEDS['simple'])
    img = seeded_randn((1, 3, 128, 128), SEEDS['simple'], 'img').cuda()
    isr = seeded_randn((1, 3, 128, 128), SEEDS['simple'], 'isr').clamp(-1, 1).cuda()
    logit = m.encode_decode(None, isr, test_cfg={'output_type': 'events'})
    assert_close(logit[..., ::8, ::8], g['simple.logit_s'], 1e-4, name='encode_decode logits (events output)')
    meta = dict(ori_shape=(96, 160, 3), flip=False)
    seg = np.stack(m.simple_test(True, image=img, night_isr=isr, img_metas=meta))
    assert seg.shape == (1, 96, 160)
    check_le('simple_test: label disagreement', 1 - (seg == g['simple.seg'].numpy()).mean(), 1e-3)
    lab = m.predict(True, image=img, night_isr=isr, img_metas=meta).cpu().numpy()
    check_le('predict: label disagreement', 1 - (lab == g['simple.seg'].numpy()).mean(), 1e-3)


def _fp_rel(got, ref):
    return max((got[:-2] - ref[:-2]).abs().max().item() / (ref[:-2].abs().max().item() + 1e-12),
               (got[-2:] - ref[-2:]).abs().max().item() / (ref[-1].abs().item() + 1e-12))


STEP_CASES = {'shared': (True, 3), 'separate': (False, 1)}


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(STEP_CASES))
@pytest.mark.parametrize('mode', ['f32', 'x3'])
def test_split_step_against_reference_fixture_gpu(mode, case):
    """train_step on one 512 x 512 pair with the reference's recorded draws injected, FlatAdamW between the iterations.  Per
    iteration and per stream, with the bounds of test_image_uda.py::test_image_step_against_reference_fixture_gpu quantity by quantity
    (the events stream takes the image stream's; the mixed ISR, which that test does not have, the bound of
    test_dacs.py::test_dacs_train_step_against_reference_fixture_gpu).  Then to three steps in all: every parameter the reference
    leaves without a gradient is bit-identical to its initial value, in the student; it is in the state dict and in the teacher."""
    from cmda_amd.optim import FlatAdamW
    _gpu()
    share, iters = STEP_CASES[case]
    g = golden('dacs_step_split.npz')
    src, tg = split_batch()
    exact = mode == 'f32'
    rt.set_compute_dtype(torch.float32)
    rt.set_gemm_x3(mode == 'x3')
    dacs = None
    try:
        dacs = build_train_model(make_cfg(share_decoder=share))
        seeded_fill(dacs.model, SEEDS['student'])
        seeded_fill(dacs.ema_model, SEEDS['teacher'])
        with torch.no_grad():
            dacs.model.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE)
            dacs.model.decode_head.conv_seg_events.weight.mul_(DACS_SEG_SCALE)
        dacs = dacs.to('cuda:0').train()
        if share:
            assert sorted(dacs.state_dict().keys()) == sorted(json.load(open(os.path.join(HERE, 'golden', 'dacs_split_keys.json'))))
        none = g[f'{case}.grad_none']
        init = {k: q.detach().cpu().clone() for k, q in dacs.model.named_parameters() if k in none}
        assert sorted(init) == sorted(none)
        opt = FlatAdamW(dacs.model, lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01)
        for it in range(3):
            p = f'{case}.it{min(it, iters - 1)}'
            cj, bl, sigma = [float(v) for v in g[f'{p}.gates']]
            cls = torch.full((1, dacs._kmax()), -1, dtype=torch.int64)
            cls[0, :g[f'{p}.classes'].numel()] = g[f'{p}.classes']
            dacs.inject_draws = dict(choice=0.0, color_jitter=cj, blur=bl, sigma=sigma, classes=cls, jitter=None,
                                     direction=DIRECT[int(cj * 10) % 2][int(cj * 100) % 2], sky=None, isr_noise=None)
            batch = dict(source={k: v.clone().cuda() for k, v in src.items()}, target={k: v.clone().cuda() for k, v in tg.items()})
            res = dacs.train_step(batch, opt)
            torch.cuda.synchronize()
            if it >= iters:
                continue   # (past the fixture's iterations: only the never-read parameters are looked at, below)
            lv = res['log_vars']
            assert sorted(lv.keys()) == sorted(g[f'{p}.log_keys']), f'{p} log_vars keys'
            names = ['decode.loss_seg', 'decode.acc_seg', 'mix.decode.loss_seg', 'mix.decode.acc_seg']
            got = torch.tensor([float(lv[k]) for k in names])
            ref = g[f'{p}.losses'].float()
            print(p, mode, 'losses', got.tolist(), 'reference', ref.tolist())
            tol_l = (1e-4 if exact else 3e-4) * (1 if it == 0 else 10)
            assert_close(got[[0, 2]], ref[[0, 2]], tol_l, name=f'{p} losses vs reference')
            check_le(f'{p} accuracies vs reference (points)', (got[[1, 3]] - ref[[1, 3]]).abs().max().item(), 0.1 if it == 0 else 0.5)
            mix = dacs.last_mix
            for s, suffix in (('image', ''), ('events', '_events')):
                q = f'{p}.{s}'
                plab = mix['pseudo_label' + suffix].cpu().view(1, 512, 512)[..., ::8, ::8].to(torch.uint8)
                agree = (plab.flatten() == g[f'{q}.pseudo_label_s'].flatten()).float().mean().item()
                check_le(f'{q} pseudo-label disagreement', 1 - agree, 1e-3 if it == 0 else 1e-2)
                check_le(f'{q} confident-pixel count rel', abs(int(mix['pseudo_count' + suffix].sum()) - int(g[f'{q}.pseudo_conf'])) /
                         max(1, int(g[f'{q}.pseudo_conf'])), 1e-3 if it == 0 else 1e-2)
                teacher = ops.upsample_logits_nchw(mix['teacher_logits'][s + '_output'], 512, 512)
                assert_close(teacher[..., ::64, ::64], g[f'{q}.teacher_s'], 1e-3 if it == 0 else 1e-2, name=f'{q} teacher logits')
                mlab = mix['mixed_lbl' + suffix].cpu().view(1, 512, 512)[..., ::8, ::8].to(torch.uint8)
                agree = (mlab.flatten() == g[f'{q}.mixed_lbl_s'].flatten()).float().mean().item()
                check_le(f'{q} mixed-label disagreement', 1 - agree, 1e-3 if it == 0 else 1e-2)
                assert_close(mix['pseudo_weight' + suffix].view(1, 512, 512)[..., ::8, ::8], g[f'{q}.mixed_weight_s'].view(1, 64, 64),
                             1e-3 if it == 0 else 1e-2, name=f'{q} mixed weight')
            assert_close(mix['mixed_img'][..., ::16, ::16], g[f'{p}.mixed_img_s'], 1e-6, name=f'{p} mixed image')
            assert_close(mix['mixed_isr'].cpu()[:, :1, ::4, ::4], g[f'{p}.mixed_isr_s'].float(), 1e-3, name=f'{p} mixed ISR')
            row = {k: i for i, k in enumerate(g[f'{case}.param_names'])}
            assert sorted(row) == sorted(k for k, _ in dacs.model.named_parameters())
            worst_g = max(_fp_rel(sample_grad(q.grad.cpu(), FP_N), g[f'{p}.grad'][row[k]]) for k, q in dacs.model.named_parameters())
            check_le(f'{p} {mode} worst gradient fingerprint error vs reference', worst_g,
                     (1.2e-2 if exact else 3e-2) if it == 0 else (0.3 if exact else 0.4))
            worst_e = max(_fp_rel(sample_grad(q.detach().cpu(), FP_N), g[f'{p}.ema'][row[k]]) for k, q in dacs.ema_model.named_parameters())
            check_le(f'{p} {mode} worst EMA fingerprint error vs reference', worst_e, 1e-3 if it == 0 else 1e-2)
        assert opt.step_count == 3
        opt.synchronize()
        torch.cuda.synchronize()
        student, teacher, sd = dict(dacs.model.named_parameters()), dict(dacs.ema_model.named_parameters()), dacs.state_dict()
        for k, v in init.items():
            assert torch.equal(student[k].detach().cpu(), v), f'{k}: never read, yet changed by three optimizer steps'
            assert 'model.' + k in sd and 'ema_model.' + k in sd
            assert_close(teacher[k], v, 1e-6, name=f'teacher copy of {k}')
    finally:
        if dacs is not None:
            dacs.inject_draws = None
        rt.set_gemm_x3(False)
        rt.set_compute_dtype(torch.float32)


@pytest.mark.gpu
def test_split_graph_replay_matches_eager_gpu():
    """three iterations eager against hipGraph replay (warm-up 1, capture at iteration 1): same losses, same gradients;
    the bounds of test_image_uda.py::test_image_graph_replay_matches_eager_gpu"""
    dev = _gpu().device
    rt.set_compute_dtype(torch.float32)
    src, tg = small_batch()
    runs = []
    for graph in (False, True):
        dacs = build_train_model(make_cfg([32, 64, 160, 256], 64))
        seeded_fill(dacs.model, 7)
        seeded_fill(dacs.ema_model, 8)
        dacs.to(dev).train()
        torch.manual_seed(11), random.seed(11), np.random.seed(11)
        if graph:
            dacs.enable_graph(warmup_iters=1)
        batch = dict(source={k: v.to(dev) for k, v in src.items()}, target={k: v.to(dev) for k, v in tg.items()})
        out = []
        for it in range(3):
            for p in dacs.model.parameters():
                if p.grad is not None:
                    p.grad.zero_()
            lv = dacs(**batch)
            torch.cuda.synchronize()
            out.append(({k: float(v) for k, v in lv.items() if 'loss' in k},
                        {n: p.grad.detach().cpu().clone() for n, p in dacs.model.named_parameters() if p.grad is not None}))
        if graph:
            assert dacs._graph is not None, 'the iteration was not captured'
        runs.append(out)
    for it, ((l_e, g_e), (l_g, g_g)) in enumerate(zip(*runs)):
        assert l_e.keys() == l_g.keys() and all(np.isfinite(v) for v in l_e.values())
        for k in l_e:
            assert_close(torch.tensor([l_g[k]]), torch.tensor([l_e[k]]), 1e-4, name=f'it{it} {k}, graph vs eager')
        assert g_e.keys() == g_g.keys() and 'decode_head.conv_seg_events.weight' in g_e and 'decode_head.conv_seg_fusion.weight' not in g_e
        worst = max((g_g[n] - q).abs().max().item() / (q.abs().max().item() + 1e-12) for n, q in g_e.items())
        check_le(f'split it{it} worst gradient rel error, graph vs eager', worst, 5e-2, strict=True)
