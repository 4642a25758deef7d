"""The ISR augmentations inside the training step (DACS: cfg['sky_mask'], cfg['isr_noise_dacs_type']) and the loader
(CityscapesICDataset: sky_mask=, isr_noise=): wiring, draws through the control block, graph replay, and the options that stay out of
scope."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_dacs as TD  # noqa: E402
from test_isr_augment import SKY, isr_noise_ref, sky_mask_ref  # noqa: E402
from weights import seeded_fill  # noqa: E402

import cmda_amd.runtime as rt  # noqa: E402
from cmda_amd import datasets as D, ops  # noqa: E402
from cmda_amd.registry import build_train_model  # noqa: E402
from conftest import check_le  # noqa: E402

H = W = 64
TYPES = {'cs2dz_image+raw-isr': dict(train_type='cs2dz_image+raw-isr', fusion='AttentionFusion', generator=False),
         'cs2dsec_image+events_together': dict(train_type='cs2dsec_image+events_together')}


def _bank():
    return torch.randint(0, 256, (2, H, W), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)


def _batch(tgt, counts=False):
    src, tg = TD.make_batch(2, H, W)
    src['label'][0, 0, 8:40, 8:48] = SKY   # sample 0: a sky blob; sample 1: five sky pixels, below the threshold of 10
    src['label'][1, 0, 20, 10:15] = SKY
    batch = dict(source={k: tgt.to(v) for k, v in src.items()}, target={k: tgt.to(v) for k, v in tg.items()})
    if counts:   # what the loader attaches next to the class set
        lab = batch['source']['label']
        lab._cmda_sky_counts = [int((src['label'][b] == SKY).sum()) for b in range(2)]
        lab._cmda_classes_key = (lab.data_ptr(), lab._version)
    return src, batch


def _build(tgt, variant, graph=False, **uda):
    rt.set_compute_dtype(torch.float32)
    torch.manual_seed(5)   # (the noise generator's key is torch.initial_seed() at construction)
    cfg = TD.make_cfg(TD.SMALL['dims'], TD.SMALL['ch'], shift_type='random', **variant)
    cfg['uda'].update(uda)
    dacs = build_train_model(cfg)
    seeded_fill(dacs.model, 7)
    seeded_fill(dacs.ema_model, 8)
    if dacs.cyclegan_itrd2en is not None:
        seeded_fill(dacs.cyclegan_itrd2en, 9)
    dacs.to(tgt.device).train()
    if graph:
        dacs.enable_graph(warmup_iters=1)
    torch.manual_seed(11), random.seed(11), np.random.seed(11)
    return dacs


def _run(dacs, batch, iters):
    outs = []
    for _ in range(iters):
        for p in dacs.model.parameters():
            if p.grad is not None:
                p.grad.zero_()
        log_vars = dacs(**batch)
        outs.append(({k: v.detach().cpu().clone() for k, v in log_vars.items()},
                     {k: v.detach().cpu().clone() for k, v in dacs.last_mix.items() if isinstance(v, torch.Tensor)}, dacs.last_draws))
    return outs


@pytest.mark.parametrize('train_type', sorted(TYPES))
def test_dacs_isr_augmentations(tgt, train_type):
    """two iterations with both options on: the student's source ISR is ops.sky_mask of the batch's ISR under the staged draws,
    extras['mixed_isr'] is ops.isr_noise of the ISR of extras['mixed_img'] at offset = iteration, the losses are finite"""
    counts = train_type == 'cs2dz_image+raw-isr'   # one type with the loader's sky counts, one with the device-side decision alone
    bank = _bank()
    dacs = _build(tgt, TYPES[train_type], sky_mask=bank, isr_noise_dacs_type='noise+blur')
    src, batch = _batch(tgt, counts)
    isr0 = src['img_self_res'].clone()
    outs = _run(dacs, batch, 2)
    assert torch.equal(batch['source']['img_self_res'].cpu(), isr0), "the loader's ISR buffer is left alone"
    for it, (log_vars, mix, d) in enumerate(outs):
        assert all(torch.isfinite(v).all() for v in log_vars.values()), log_vars
        assert len(d['sky']) == 2 and len(d['isr_noise']) == 2
        if counts:
            assert torch.equal(d['sky'][1]['rows'], torch.arange(H, dtype=torch.int32)), 'below 10 sky pixels the draws stop early'
        prm, rows, cols = (tgt.to(t) for t in ops.sky_mask_params(d['sky']))
        want = ops.sky_mask(batch['source']['label'], batch['source']['img_self_res'], tgt.to(bank), prm, rows, cols).cpu()
        assert torch.equal(mix['day_isr'], want), f'iteration {it}: source ISR'
        ref, _, _ = sky_mask_ref(src['label'], isr0, bank, d['sky'])
        check_le(f'{train_type} it {it}: source ISR against the restatement', (mix['day_isr'] - ref).abs().max().item(), 1e-6)
        assert torch.equal(mix['day_isr'][1], isr0[1]) and not torch.equal(mix['day_isr'][0], isr0[0])
        gray = ops.isr_gray(tgt.to(mix['mixed_img']))
        clean = ops.isr_from_gray(gray, TD.ISR['val_range'], TD.ISR['_threshold'], TD.ISR['_clip_range'], TD.ISR['shift_pixel'], d['direction'])
        nprm = tgt.to(ops.isr_noise_params(d['isr_noise']))
        want = ops.isr_noise(clean, nprm, 'noise+blur', seed=dacs.isr_noise_seed, offset=it).cpu()
        assert torch.equal(mix['mixed_isr'], want), f'iteration {it}: mixed ISR'
        fields = ops.randn_fields(2, H, W, dacs.isr_noise_seed, it, device=tgt.device).cpu()
        ref = isr_noise_ref(clean.cpu(), d['isr_noise'], 'noise+blur', fields)
        check_le(f'{train_type} it {it}: mixed ISR against the restatement', (mix['mixed_isr'] - ref).abs().max().item(), 1e-6)
    assert not torch.equal(outs[0][1]['mixed_isr'], outs[1][1]['mixed_isr'])


def test_dacs_options_off_is_todays_iteration(tgt):
    """sky_mask=None and isr_noise_dacs_type='' against a configuration that names neither: the same control block, draws, extras"""
    variant = TYPES['cs2dz_image+raw-isr']
    res = []
    for uda in (dict(), dict(sky_mask=None, isr_noise_dacs_type='')):
        dacs = _build(tgt, variant, **uda)
        assert dacs.sky_bank is None and dacs.isr_noise_dacs_type == ''
        _, batch = _batch(tgt)
        res.append((_run(dacs, batch, 1)[0], dacs._ctl['dev'].numel(), set(dacs._ctl['d'])))
    (lv0, mix0, d0), n0, k0 = res[0]
    (lv1, mix1, d1), n1, k1 = res[1]
    assert n0 == n1 and k0 == k1 and 'sky_prm' not in k1 and 'noise_prm' not in k1, 'the control block is unchanged'
    assert d1['sky'] is None and d1['isr_noise'] is None and 'day_isr' not in mix1
    assert set(mix0) == set(mix1) and set(lv0) == set(lv1)
    for k in ('mixed_img', 'mixed_isr', 'mixed_lbl', 'classes'):
        assert torch.equal(mix0[k], mix1[k]), k
    for k in lv0:   # (BatchNorm statistics are summed with float atomics: the losses agree to round-off, not to the bit)
        check_le(f'options off: {k}', (lv0[k] - lv1[k]).abs().item(), 1e-5 * max(1.0, lv0[k].abs().item()))


@pytest.mark.gpu
@pytest.mark.parametrize('train_type', sorted(TYPES))
def test_dacs_isr_augmentations_graph_replay_gpu(train_type):
    """iteration 0 eager, iterations 1-2 replayed: the same source ISR and mixed ISR as three eager iterations under the same seeds
    (the draws and the noise offset travel through the control block)"""
    from conftest import Target
    from cmda_amd import _lib
    _lib._unbind_for_tests()
    if not torch.cuda.is_available():
        pytest.skip('no GPU on this machine')
    tgt = Target('gpu')
    runs = []
    for graph in (False, True):
        dacs = _build(tgt, TYPES[train_type], graph=graph, sky_mask=_bank(), isr_noise_dacs_type='noise+blur')
        _, batch = _batch(tgt)
        runs.append(_run(dacs, batch, 3))
        assert (dacs._graph is not None) == graph
    for it, ((lv_e, mix_e, d_e), (lv_g, mix_g, d_g)) in enumerate(zip(*runs)):
        assert d_e['sky'][0]['k'] == d_g['sky'][0]['k'] and d_e['isr_noise'] == d_g['isr_noise']
        assert torch.equal(mix_e['day_isr'], mix_g['day_isr']), f'iteration {it}: source ISR'
        assert torch.equal(mix_e['mixed_isr'], mix_g['mixed_isr']), f'iteration {it}: mixed ISR'
        assert torch.isfinite(lv_g['mix.decode.loss_seg']) and torch.isfinite(lv_g['decode.loss_seg'])
    assert not torch.equal(runs[1][1][1]['mixed_isr'], runs[1][2][1]['mixed_isr']), 'every replay sees a new offset'


def test_dacs_bank_of_another_size_raises(tgt):
    dacs = _build(tgt, TYPES['cs2dz_image+raw-isr'], sky_mask=torch.zeros(2, H, W + 8, dtype=torch.uint8))
    _, batch = _batch(tgt)
    with pytest.raises(ValueError, match='noise bank'):
        dacs(**batch)


def test_dacs_bank_from_directory(tmp_path):
    from PIL import Image
    bank = _bank()
    Image.fromarray(bank[0].numpy()).save(tmp_path / 'a.png')
    np.save(tmp_path / 'b.npy', bank[1].numpy())
    got = ops.load_noise_bank(str(tmp_path))
    names = os.listdir(tmp_path)
    assert torch.equal(got, torch.stack([bank[0] if n == 'a.png' else bank[1] for n in names])), 'os.listdir order'
    with pytest.raises(ValueError):
        ops.load_noise_bank(torch.zeros(2, 4, 4))


# ---- the loader --------------------------------------------------------------------------------------------------------------------
def _dataset(tgt, **kw):
    return D.build_dataset(dict(type='CityscapesICDataset', raw_size=(256, 128), image_resize_size=(128, 64), image_crop_size=(64, 64),
                                outputs={'image', 'label', 'img_self_res'}, synthetic_length=4, device=tgt.device, **kw))


def _sky_labels(ds):
    """the synthetic labels carry no fixed sky share: relabel class 3 as sky so that both sides of the threshold occur"""
    raw = ds.raw

    def with_sky(idx):
        now, prev, lab = raw(idx)
        lab = lab.clone()
        lab[lab == SKY] = 11
        lab[lab == 3] = SKY
        return now, prev, lab
    ds.raw = with_sky
    return ds


def test_loader_isr_augmentations(tgt):
    bank = _bank()
    idx = [0, 1, 2]

    def make(**kw):
        torch.manual_seed(3)
        return _sky_labels(_dataset(tgt, **kw))

    def seeded(fn):
        torch.manual_seed(9), random.seed(9)
        return fn()
    plain = seeded(lambda: make().get_batch(idx))
    ds = make(sky_mask=bank, isr_noise=True)
    aug = seeded(lambda: ds.get_batch(idx))
    draws = ds.last_isr_draws
    assert torch.equal(aug['image'], plain['image']) and torch.equal(aug['label'], plain['label']), 'the same crops'
    lab = aug['label'].cpu()
    assert aug['label']._cmda_sky_counts == [int((lab[b] == SKY).sum()) for b in range(3)]
    assert plain['label']._cmda_sky_counts == aug['label']._cmda_sky_counts
    x = aug['img_self_res'].cpu()
    assert x.shape == (3, 3, 64, 64) and x.abs().max() <= 1 and torch.isfinite(x).all()
    # where the restatement says: sky mask, then noise + blur with the kernel's fields of (seed, batch 0)
    ref, _, _ = sky_mask_ref(lab, plain['img_self_res'].cpu(), bank, draws['sky'])
    fields = ops.randn_fields(3, 64, 64, ds.isr_noise_seed, 0, device=tgt.device).cpu()
    ref = isr_noise_ref(ref, draws['isr_noise'], 'noise+blur', fields)
    check_le('loader img_self_res against the restatement', (x - ref).abs().max().item(), 1e-6)
    assert torch.equal(x != plain['img_self_res'].cpu(), ref != plain['img_self_res'].cpu()), 'changed exactly where the restatement changes it'
    assert (x != plain['img_self_res'].cpu()).any()
    # __getitem__ is get_batch of one sample
    a = seeded(lambda: make(sky_mask=bank, isr_noise=True).get_batch([2]))
    b = seeded(lambda: make(sky_mask=bank, isr_noise=True)[2])
    for k in ('image', 'label', 'img_self_res'):
        assert torch.equal(a[k][0], b[k]), k
    # each alone
    ds = make(sky_mask=bank)
    only_sky = seeded(lambda: ds.get_batch(idx))['img_self_res'].cpu()
    assert ds.last_isr_draws['isr_noise'] is None
    ref, _, _ = sky_mask_ref(lab, plain['img_self_res'].cpu(), bank, ds.last_isr_draws['sky'])
    check_le('loader sky mask alone', (only_sky - ref).abs().max().item(), 1e-6)
    with pytest.raises(ValueError, match='noise bank'):
        _dataset(tgt, sky_mask=torch.zeros(2, 64, 72, dtype=torch.uint8))


def test_out_of_scope_options_still_raise(tgt):
    for kw in (dict(isr_cow_mask=True), dict(random_flare='flares/'), dict(high_resolution_isr=True), dict(shift_3_channel=True)):
        with pytest.raises(AssertionError):
            _dataset(tgt, **kw)
    cfg = TD.make_cfg(TD.SMALL['dims'], TD.SMALL['ch'])
    for uda in (dict(isr_noise_dacs_type='cow'), dict(train_type='cs2dz_image+d2n-isr'), dict(cyclegan_light_path='x', train_type='cs2dz_image')):
        bad = dict(cfg, uda=dict(cfg['uda'], **uda))
        with pytest.raises((AssertionError, ValueError)):
            build_train_model(bad)
    image_only = TD.make_cfg(TD.SMALL['dims'], TD.SMALL['ch'])
    with pytest.raises(AssertionError):
        build_train_model(dict(image_only, uda=dict(image_only['uda'], train_type='cs2dsec_image', mixed_image_to_mixed_isr=False,
                                                    sky_mask=_bank())))
