"""The three-channel ISR (`shift_3_channel` / list-form `isr_parms`) and the cow mask where users meet them: the DACS training step,
DarkZurichICDataset and CityscapesICDataset."""
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_dacs as TD  # noqa: E402
import test_isr_augment_uda as TU  # noqa: E402
from test_cow_mask import BAND, BAND_SHARE, restate  # noqa: E402
from test_isr_augment import SKY, isr_noise_ref, sky_mask_ref  # noqa: E402

from cmda_amd import datasets as D, ops, pipeline as pl  # noqa: E402
from cmda_amd.registry import build_train_model  # noqa: E402
from conftest import assert_close, check_le  # noqa: E402
from oracle import uda as ouda  # noqa: E402

H = W = TU.H
VARIANT = TU.TYPES['cs2dz_image+raw-isr']
DACS3 = D.ISR3_PRESETS['dacs']
FLAG = dict(shift_3_channel=True, isr_parms='')   # (the helpers' configuration names a one-channel isr_parms: the flag excludes it)


def oracle_isr3_of_gray(gray_u8, preset):
    """uint8 [H,W] -> [3,H,W]: the reference's loop over get_image_change_from_pil, direction 'rightdown'"""
    return torch.cat([ouda.image_change(gray_u8.numpy(), p['shift_pixel'], p['val_range'], p['_threshold'], p['_clip_range'])
                      for p in preset])


def oracle_mixed_isr3(mixed_img, preset):
    return torch.stack([torch.cat([ouda.mixed_image_to_isr(mixed_img[b:b + 1], p['shift_pixel'], p['val_range'], p['_threshold'],
                                                           p['_clip_range'], 'rightdown')[0, :1] for p in preset])
                        for b in range(mixed_img.shape[0])])


def _distinct(x, what):
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not torch.equal(x[:, a], x[:, b]), f'{what}: channels {a} and {b} coincide'


def _same_draws(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


_RUNS = {}


def _runs(tgt):
    """the eager runs the DACS tests below share (a small model, but an iteration on the emulator takes most of a minute): no key,
    flag off, flag on, list form -- each built and seeded alike"""
    if tgt.kind not in _RUNS:
        _, batch = TU._batch(tgt)
        r = {}
        for name, uda, iters in (('none', dict(), 2), ('false', dict(shift_3_channel=False), 1), ('flag', FLAG, 2),
                                 ('list', dict(isr_parms=[dict(p) for p in DACS3]), 1)):
            dacs = TU._build(tgt, VARIANT, **uda)
            r[name] = (TU._run(dacs, batch, iters), dacs._ctl['dev'].numel(), set(dacs._ctl['d']), dacs.isr3)
        _RUNS[tgt.kind] = r
    return _RUNS[tgt.kind]


def test_dacs_three_channel_isr(tgt):
    r = _runs(tgt)
    off, flag, lst = r['none'][0], r['flag'][0], r['list'][0]
    assert 'isr3_prm' in r['flag'][2] and r['flag'][3] == DACS3
    for it, ((lv, mix, d), (_, mix_off, d_off)) in enumerate(zip(flag, off)):
        assert all(torch.isfinite(v).all() for v in lv.values()), lv
        _same_draws(d, d_off)
        assert torch.equal(mix['mixed_img'], mix_off['mixed_img'])
        assert mix['mixed_isr'].shape == (2, 3, H, W)
        _distinct(mix['mixed_isr'], f'iteration {it}')
        assert_close(mix['mixed_isr'], oracle_mixed_isr3(mix['mixed_img'], DACS3), 1e-5, atol=1e-6, name=f'it {it}: three-channel mixed ISR',
                     outlier_frac=5e-3, outlier_rtol=2.0)
        assert torch.equal(mix_off['mixed_isr'][:, 0], mix_off['mixed_isr'][:, 2]), 'flag off: one channel, repeated'
    # the list form holding the preset is the flag
    _same_draws(flag[0][2], lst[0][2])
    assert torch.equal(flag[0][1]['mixed_isr'], lst[0][1]['mixed_isr'])


def test_dacs_flag_off_is_todays_iteration(tgt):
    r = _runs(tgt)
    ((lv0, mix0, d0), n0, k0, i0), ((lv1, mix1, d1), n1, k1, i1) = (r['none'][0][0],) + r['none'][1:], (r['false'][0][0],) + r['false'][1:]
    assert i0 is None and i1 is None
    assert n0 == n1 and k0 == k1 and 'isr3_prm' not in k1, 'the control block is unchanged'
    _same_draws(d0, d1)
    assert set(mix0) == set(mix1) and set(lv0) == set(lv1)
    for k in ('mixed_img', 'mixed_isr', 'mixed_lbl', 'classes'):
        assert torch.equal(mix0[k], mix1[k]), k
    for k in lv0:   # (BatchNorm statistics are summed with float atomics: the losses agree to round-off, not to the bit)
        check_le(f'flag off: {k}', (lv0[k] - lv1[k]).abs().item(), 1e-5 * max(1.0, lv0[k].abs().item()))


def test_dacs_three_channel_isr_with_noise(tgt):
    """dacs.py:753-755: channel 0 of the three-channel ISR through add_noise_on_isr, the result on all three channels"""
    _, batch = TU._batch(tgt)
    dacs = TU._build(tgt, VARIANT, isr_noise_dacs_type='noise', **FLAG)
    prm3 = ops.isr_multi_params(DACS3, 'rightdown', tgt.device)
    for it, (lv, mix, d) in enumerate(TU._run(dacs, batch, 2)):
        x = mix['mixed_isr']
        assert torch.equal(x[:, 0], x[:, 1]) and torch.equal(x[:, 0], x[:, 2])
        clean = ops.isr_multi(ops.isr_gray(tgt.to(mix['mixed_img'])), DACS3[0]['val_range'], prm3, 3)
        want = ops.isr_noise(clean, tgt.to(ops.isr_noise_params(d['isr_noise'])), 'noise', seed=dacs.isr_noise_seed, offset=it).cpu()
        assert torch.equal(x, want), f'iteration {it}'
        assert not torch.equal(x[:, 0], clean[:, 0].cpu())
        assert all(torch.isfinite(v).all() for v in lv.values())


def test_dacs_three_channel_isr_refusals():
    cfg = TD.make_cfg(TD.SMALL['dims'], TD.SMALL['ch'], **VARIANT)
    with pytest.raises(AssertionError):   # dacs.py:167-168 (the helpers' configuration names isr_parms)
        build_train_model(dict(cfg, uda=dict(cfg['uda'], shift_3_channel=True)))
    with pytest.raises(AssertionError):
        build_train_model(dict(cfg, uda=dict(cfg['uda'], shift_3_channel=True, isr_parms=[dict(p) for p in DACS3])))
    with pytest.raises(AssertionError):   # two value ranges in one list
        build_train_model(dict(cfg, uda=dict(cfg['uda'], isr_parms=[DACS3[0], DACS3[1], D.ISR3_PRESETS['day'][2]])))
    image = TD.make_cfg(TD.SMALL['dims'], TD.SMALL['ch'])
    for uda in (FLAG, dict(isr_parms=[dict(p) for p in DACS3])):
        with pytest.raises(AssertionError):
            build_train_model(dict(image, uda=dict(image['uda'], train_type='cs2dsec_image', mixed_image_to_mixed_isr=False, **uda)))


@pytest.mark.gpu
def test_dacs_three_channel_isr_graph_replay_gpu():
    """iteration 0 eager, iterations 1-2 replayed: the same three-channel mixed ISR as three eager iterations under the same seeds"""
    from conftest import Target
    from cmda_amd import _lib
    _lib._unbind_for_tests()
    if not torch.cuda.is_available():
        pytest.skip('no GPU on this machine')
    tgt = Target('gpu')
    runs = []
    for graph in (False, True):
        dacs = TU._build(tgt, VARIANT, graph=graph, **FLAG)
        _, batch = TU._batch(tgt)
        runs.append(TU._run(dacs, batch, 3))
        assert (dacs._graph is not None) == graph
    for it, ((lv_e, mix_e, d_e), (lv_g, mix_g, d_g)) in enumerate(zip(*runs)):
        _same_draws(d_e, d_g)
        assert torch.equal(mix_e['mixed_isr'], mix_g['mixed_isr']), f'iteration {it}: mixed ISR'
        _distinct(mix_g['mixed_isr'], f'replay {it}')
        assert torch.isfinite(lv_g['mix.decode.loss_seg']) and torch.isfinite(lv_g['decode.loss_seg'])


# ---- Dark Zurich loader --------------------------------------------------------------------------------------------------------------
DZ = dict(type='DarkZurichICDataset', raw_size=(256, 144), image_resize_size=(128, 72), image_crop_size=(64, 64), synthetic_length=4)
DZ_SEED = 0   # three samples whose (flip, x, y) cover both flips and odd and even offsets (asserted below)


def _dz(tgt, **kw):
    return D.build_dataset(dict(DZ, device=tgt.device, **kw))


def _dz_draws(n):
    random.seed(DZ_SEED)
    return [(int(random.random() < 0.5), random.randint(0, 128 - 64), random.randint(0, 72 - 64)) for _ in range(n)]


def _dz_gray(ds, idx):
    frames = torch.stack([ds.raw(i)[0] for i in idx]).to(ds.device)
    return pl.pil_resize_u8(frames, pl.make_samp(len(idx), ds.device), (256, 144), (128, 72), want_u8=True, want_gray=True,
                            norm=(pl.IMAGENET_MEAN, pl.IMAGENET_STD))['gray']


def test_dark_zurich_three_channel_isr(tgt):
    idx = [0, 1, 2]
    draws = _dz_draws(3)
    assert {d[0] for d in draws} == {0, 1} and {d[1] % 2 for d in draws} == {0, 1} and {d[2] % 2 for d in draws} == {0, 1}, draws
    for kw, preset in ((dict(shift_3_channel=True), 'night'), (dict(shift_3_channel=True, dz_isr_data_type='new_night'), 'new_night'),
                       (dict(isr_parms=D.ISR3_PRESETS['day']), 'day')):
        ds = _dz(tgt, **kw)
        gray = _dz_gray(ds, idx).cpu()
        random.seed(DZ_SEED)
        got = ds.get_batch(idx)['night_isr'].cpu()
        assert got.shape == (3, 3, 64, 64)
        _distinct(got, preset)
        for b, (f, x, y) in enumerate(draws):
            ref = oracle_isr3_of_gray(gray[b], D.ISR3_PRESETS[preset])[:, y:y + 64, x:x + 64]
            ref = torch.flip(ref, dims=[-1]) if f else ref
            assert_close(got[b], ref, 2e-6, atol=2e-7, name=f'dark zurich {preset} sample {b}')
    night = _dz(tgt, shift_3_channel=True)
    random.seed(DZ_SEED)
    a = night.get_batch(idx)['night_isr']
    random.seed(DZ_SEED)
    b = _dz(tgt, shift_3_channel=True, dz_isr_data_type='new_night').get_batch(idx)['night_isr']
    assert not torch.equal(a.cpu(), b.cpu()), 'dz_isr_data_type picks the preset'
    # test mode: the whole resized frame
    ds = _dz(tgt, shift_3_channel=True, test_mode=True, outputs={'image', 'night_isr', 'label'})
    full = ds.get_batch([1])['night_isr'].cpu()
    assert full.shape == (1, 3, 72, 128)
    assert_close(full[0], oracle_isr3_of_gray(_dz_gray(ds, [1]).cpu()[0], D.ISR3_PRESETS['night']), 2e-6, atol=2e-7, name='dark zurich test mode')
    with pytest.raises(AssertionError):
        _dz(tgt, shift_3_channel=True, isr_parms=D.ISR3_PRESETS['night'])
    with pytest.raises(AssertionError):
        _dz(tgt, shift_3_channel=True, high_resolution_isr=True)
    with pytest.raises(AssertionError):
        _dz(tgt, auto_threshold=True)


def test_dark_zurich_flag_off_is_todays_batch(tgt):
    idx = [0, 1, 2]
    ds = _dz(tgt, shift_3_channel=False)
    random.seed(DZ_SEED)
    got = ds.get_batch(idx)
    gray = _dz_gray(ds, idx)
    p = ds.isr_parms
    for b, (f, x, y) in enumerate(_dz_draws(3)):   # the one-channel path: ISR of the whole frame, slice, flip
        v = ops.isr_from_gray(gray[b:b + 1], p['val_range'], p['_threshold'], p['_clip_range'], p['shift_pixel'], 'rightdown')
        v = v[:, :, y:y + 64, x:x + 64]
        v = torch.flip(v, dims=[-1]) if f else v
        assert torch.equal(got['night_isr'][b].cpu(), v[0].cpu()), b
    assert torch.equal(got['night_isr'][:, 0].cpu(), got['night_isr'][:, 2].cpu())


# ---- Cityscapes loader -----------------------------------------------------------------------------------------------------------------
NEW_DAY = D.ISR3_PRESETS['new_day']


def _cs(tgt, crop=64, **kw):
    torch.manual_seed(3)
    ds = D.build_dataset(dict(type='CityscapesICDataset', raw_size=(4 * crop, 2 * crop), image_resize_size=(2 * crop, crop),
                              image_crop_size=(crop, crop), outputs={'image', 'label', 'img_self_res'}, synthetic_length=4,
                              device=tgt.device, **kw))
    return TU._sky_labels(ds)


def _seeded(fn):
    torch.manual_seed(9), random.seed(9)
    return fn()


def test_cityscapes_three_channel_isr(tgt):
    idx = [0, 1, 2]
    one = _seeded(lambda: _cs(tgt).get_batch(idx))
    plain = _seeded(lambda: _cs(tgt, isr_parms=NEW_DAY).get_batch(idx))
    assert torch.equal(plain['image'], one['image']) and torch.equal(plain['label'], one['label']), 'the same crops'
    x0 = plain['img_self_res'].cpu()
    assert x0.shape == (3, 3, 64, 64)
    _distinct(x0, 'plain')
    # the ISR of the CROPPED image (cityscapes_ic.py:224-230): the gray map of the loader's own resize / crop / flip under the same draws
    ds = _cs(tgt, isr_parms=NEW_DAY)
    random.seed(9)
    dec = [ds.draw_decisions() for _ in idx]
    samp = pl.make_samp(3, ds.device, out_x0=[d[1] for d in dec], out_y0=[d[2] for d in dec], flip_out=[d[0] for d in dec])
    now = torch.stack([ds.raw(i)[0] for i in idx]).to(ds.device)
    res = pl.pil_resize_u8(now, samp, (256, 128), (128, 64), (64, 64), norm=(pl.IMAGENET_MEAN, pl.IMAGENET_STD), want_gray=True)
    assert torch.equal(res['f'], plain['image'])
    gray = res['gray'].cpu()
    for b in range(3):
        assert_close(x0[b], oracle_isr3_of_gray(gray[b], NEW_DAY), 2e-6, atol=2e-7, name=f'cityscapes new_day sample {b}')
    # sky mask: channels treated separately
    bank = TU._bank()
    ds = _cs(tgt, isr_parms=NEW_DAY, sky_mask=bank)
    sky = _seeded(lambda: ds.get_batch(idx))['img_self_res'].cpu()
    lab = plain['label'].cpu()
    assert any(int((lab[b] == SKY).sum()) >= 10 for b in range(3))
    for c in range(3):
        ref, _, _ = sky_mask_ref(lab, x0[:, c:c + 1].contiguous(), bank, ds.last_isr_draws['sky'])
        check_le(f'three-channel sky mask, channel {c}', (sky[:, c:c + 1] - ref).abs().max().item(), 1e-6)
    assert not torch.equal(sky, x0)
    # noise: a field of its own per channel
    ds = _cs(tgt, isr_parms=NEW_DAY, isr_noise=True)
    noisy = _seeded(lambda: ds.get_batch(idx))['img_self_res'].cpu()
    fields = ops.randn_fields(9, 64, 64, ds.isr_noise_seed, 0, device=tgt.device).cpu()
    draws = [d for d in ds.last_isr_draws['isr_noise'] for _ in range(3)]
    ref = isr_noise_ref(x0.view(9, 1, 64, 64), draws, 'noise+blur', fields).view(3, 3, 64, 64)
    check_le('three-channel loader noise against the restatement', (noisy - ref).abs().max().item(), 1e-6)
    assert torch.equal(noisy != x0, ref != x0), 'changed exactly where the restatement changes it'
    _distinct(noisy - x0, 'noise difference')
    # __getitem__ is get_batch of one sample
    a = _seeded(lambda: _cs(tgt, isr_parms=NEW_DAY, isr_noise=True, sky_mask=bank).get_batch([2]))
    b = _seeded(lambda: _cs(tgt, isr_parms=NEW_DAY, isr_noise=True, sky_mask=bank)[2])
    for k in ('image', 'label', 'img_self_res'):
        assert torch.equal(a[k][0], b[k]), k
    # the reference's flag spelling stays refused here, and says what to write instead
    with pytest.raises(AssertionError, match='ISR3_PRESETS'):
        _cs(tgt, shift_3_channel=True)
    with pytest.raises(AssertionError):
        _cs(tgt, isr_parms=NEW_DAY[:2])
    with pytest.raises(AssertionError):
        _cs(tgt, isr_parms=[NEW_DAY[0], NEW_DAY[1], D.ISR3_PRESETS['day'][2]])


@pytest.mark.parametrize('three', [True, False])
def test_cityscapes_cow_mask(tgt, three):
    idx = [0, 1]
    kw = dict(isr_parms=NEW_DAY) if three else {}
    plain = _seeded(lambda: _cs(tgt, crop=128, **kw).get_batch(idx))
    x0 = plain['img_self_res'].cpu()
    ds = _cs(tgt, crop=128, isr_cow_mask=True, **kw)
    got = _seeded(lambda: ds.get_batch(idx))
    assert torch.equal(got['image'], plain['image'])
    x = got['img_self_res'].cpu()
    cow = ds.last_isr_draws['cow']
    assert len(cow) == 2 and ds.last_isr_draws['sky'] is None and ds.last_isr_draws['isr_noise'] is None
    torch.manual_seed(9)   # per sample torch.randn([1]).uniform_ twice, nothing else from torch's generator in between
    assert [ops.draw_cow_mask() for _ in idx] == cow
    taps, tf = ops.cow_mask_params(cow)
    field = ops.cow_field(2, 128, 128, ds.isr_noise_seed, 0, device=tgt.device).cpu()
    smooth, thr, std = restate(field, taps, tf)
    for b in range(2):
        band = (smooth[b] - thr[b]).abs() <= BAND * std[b]
        check_le(f'loader cow mask [{b}] share of pixels in the threshold band', band.float().mean().item(), BAND_SHARE)
        keep = smooth[b] <= thr[b]
        check_le(f'loader cow mask [{b}] |kept share - 0.7|', abs(keep.float().mean().item() - 0.7), 0.12)
        for c in range(3):
            changed, want = x[b, c] != x0[b, c], ~keep & (x0[b, c] != 0)
            assert torch.equal(changed[~band], want[~band]), f'sample {b} channel {c}: changed exactly where the restatement drops'
            assert torch.equal(x[b, c][~changed], x0[b, c][~changed]) and (x[b, c][changed] == 0).all()
        dropped = [(x[b, c] == 0) & (x0[b, c] != 0) for c in range(3)]
        common = (x0[b] != 0).all(0)
        assert torch.equal(dropped[0][common], dropped[1][common]) and torch.equal(dropped[0][common], dropped[2][common]), 'one mask'
    # the second batch takes the next offset
    ds.get_batch(idx)
    assert ds._cow_calls == 2
    # __getitem__ is get_batch of one sample
    a = _seeded(lambda: _cs(tgt, crop=128, isr_cow_mask=True, **kw).get_batch([1]))
    b = _seeded(lambda: _cs(tgt, crop=128, isr_cow_mask=True, **kw)[1])
    assert torch.equal(a['img_self_res'][0], b['img_self_res'])
    with pytest.raises(AssertionError, match='98'):
        _cs(tgt, crop=64, isr_cow_mask=True)
