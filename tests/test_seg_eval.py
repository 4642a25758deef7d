"""On-device validation: the fused evaluation tail (`ops.seg_predict`: up-sample (+ rescale) + flip-back + arg-max + confusion counters
in one launch), `ops.confusion_update`, `metrics.ConfusionMeter`, the segmentors' `predict` and `distributed_evaluate(on_device=True)`.
The checker is plain torch on CPU (fp32, near-ties decided in float64), the shipped `simple_test` path, and the reference's own metric
outputs (tests/golden/metrics.npz)."""
import functools
import os
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
from weights import DACS_CH, DACS_DIMS, DACS_SEG_SCALE, seeded_fill, seeded_randn  # noqa: E402

import cmda_amd  # noqa: E402,F401
import cmda_amd.runtime as rt  # noqa: E402
from cmda_amd import _lib, metrics, ops, segmentors, uda  # noqa: E402
from cmda_amd._lib import CmdaError, c_i32, c_i64, ptr  # noqa: E402
from cmda_amd.registry import build_segmentor  # noqa: E402
from conftest import check_le  # noqa: E402

SEED = 2024
NAMES = ('aAcc', 'mIoU', 'mAcc', 'IoU', 'Acc')


def _sync(tgt):
    if tgt.kind == 'gpu':
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# seg_predict against torch
# (B, h, w, nc) -> (H, W) -> (OH, OW), flips
CASES = {
    'one_stage': ((2, 11, 16, 19), (44, 64), (44, 64), (0, 1, 2)),        # whole tiles
    'two_stage': ((1, 11, 16, 19), (44, 64), (48, 70), (0, 1, 2)),        # non-integer second ratio, partial tiles
    'nc32': ((1, 5, 18, 32), (19, 70), (19, 70), (0, 1, 2)),              # nc at the limit, non-integer ratio, partial tiles both ways
    'down': ((1, 40, 160, 5), (10, 40), (10, 40), (0, 1, 2)),             # down-sampling: the patch exceeds the LDS budget, un-staged path
    'eval_size': ((1, 110, 160, 19), (440, 640), (440, 640), (0, 1)),     # the DSEC evaluation size
}
CASE_FLIPS = [(name, flip) for name, c in CASES.items() for flip in c[3]]


@functools.lru_cache(maxsize=None)
def _logits(name):
    shape = CASES[name][0]
    return torch.randn(shape, generator=torch.Generator().manual_seed(SEED + sorted(CASES).index(name))) * 4


def _torch_s2(logits, hw, out_hw, dtype):
    s = F.interpolate(logits.permute(0, 3, 1, 2).to(dtype), size=hw, mode='bilinear', align_corners=False)
    if tuple(out_hw) != tuple(hw):
        s = F.interpolate(s, size=out_hw, mode='bilinear', align_corners=False)
    return s


def _flip(t, flip):
    return t if flip == 0 else t.flip(dims=(-1,) if flip == 1 else (-2,))


@functools.lru_cache(maxsize=None)
def _torch_reference(name):
    """(fp32 labels before the flip-back: argmax(softmax(S2)), near-tie mask from float64) -- computed once per case"""
    _, hw, out_hw, _ = CASES[name]
    lg = _logits(name)
    s32 = _torch_s2(lg, hw, out_hw, torch.float32)
    lab = torch.softmax(s32, dim=1).argmax(dim=1)
    assert torch.equal(lab, s32.argmax(dim=1))          # the soft-max is monotone: skipping it changes no label of the reference
    s64 = _torch_s2(lg, hw, out_hw, torch.float64)
    top2 = s64.topk(2, dim=1).values
    near = (top2[:, 0] - top2[:, 1]) < 1e-5 * lg.abs().max().double()
    assert torch.equal(lab[~near], s64.argmax(dim=1)[~near])
    return lab, near


@pytest.mark.parametrize('name,flip', CASE_FLIPS)
def test_seg_predict_matches_torch(tgt, name, flip):
    """labels of the fused kernel = torch's interpolate (once or twice) + softmax + flip + argmax at every pixel whose float64 top-2
    gap is at least 1e-5 * max|logits| (about 100 ulp of the scores); at most 1e-3 of the pixels may be that close"""
    _, hw, out_hw, _ = CASES[name]
    lab, near = _torch_reference(name)
    got = ops.seg_predict(tgt.to(_logits(name)), hw[0], hw[1], out_hw, flip)
    _sync(tgt)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(lab.shape)
    check_le(f'{name}: near-tie share', near.double().mean().item(), 1e-3)
    want, skip = _flip(lab, flip), _flip(near, flip)
    bad = (got.cpu().long() != want) & ~skip
    assert int(bad.sum()) == 0, f'{name} flip {flip}: {int(bad.sum())} labels differ outside near-ties'


@pytest.mark.parametrize('name', ['two_stage', 'nc32'])
def test_seg_predict_equals_existing_path(tgt, name):
    """the same arithmetic as the shipped path: argmax(softmax(flip(upsample_logits_nchw twice))) of `inference`, equal wherever the
    two largest fp32 soft-max values of that path are not bitwise equal"""
    _, hw, out_hw, flips = CASES[name]
    lg = tgt.to(_logits(name))
    old = segmentors._resize_logits(ops.upsample_logits_nchw(lg, hw[0], hw[1]), out_hw)
    for flip in flips:
        prob = torch.softmax(_flip(old, flip), dim=1)
        top2 = prob.topk(2, dim=1).values
        tie = (top2[:, 0] == top2[:, 1]).cpu()
        got = ops.seg_predict(lg, hw[0], hw[1], out_hw, flip)
        _sync(tgt)
        check_le(f'{name} flip {flip}: tied share of the old path', tie.double().mean().item(), 1e-3)
        assert torch.equal(got.cpu().long()[~tie], prob.argmax(dim=1).cpu()[~tie])


# ---------------------------------------------------------------------------------------------------------------------------
# confusion counters
def _gold():
    return {k: v for k, v in np.load(os.path.join(HERE, 'golden', 'metrics.npz')).items()}


def test_confusion_matches_reference_golden(tgt):
    """tests/golden/metrics.npz = outputs of the reference's own mmseg/core/evaluation/metrics.py"""
    g, nc = _gold(), 19
    preds = [torch.from_numpy(g[f'pred{i}'].astype(np.int64)) for i in range(3)]
    gts = [torch.from_numpy(g[f'gt{i}'].astype(np.int64)) for i in range(3)]
    meter = metrics.ConfusionMeter(nc, 255, device=tgt.device)
    for i, (p, t) in enumerate(zip(preds, gts)):     # device int64, host int64 (moved by the meter), numpy uint8
        if i == 0:
            meter.update(tgt.to(p), tgt.to(t))
        elif i == 1:
            meter.update(p, t)
        else:
            meter.update(p.numpy().astype(np.uint8), t.numpy().astype(np.uint8))
    assert meter.conf.dtype == torch.int64 and tuple(meter.conf.shape) == (nc + 1, nc) and meter.conf.device.type == tgt.device.type
    for k, v in zip(('inter', 'union', 'area_pred', 'area_label'), meter.areas()):
        assert v.dtype == torch.float64 and np.array_equal(v.cpu().numpy(), g['tot_' + k].astype(np.float64)), k
    r = meter.compute()
    for k in ('aAcc', 'IoU', 'Acc'):
        np.testing.assert_allclose(r[k].cpu().numpy(), g['m_' + k], rtol=1e-6, equal_nan=True, err_msg=k)   # the reference is fp32
    ref = metrics.mean_iou(preds, gts, nc, 255)
    r0, ref0 = meter.compute(nan_to_num=0), metrics.mean_iou(preds, gts, nc, 255, nan_to_num=0)
    for k in NAMES:
        np.testing.assert_allclose(r[k].cpu().numpy(), ref[k].numpy(), rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
        np.testing.assert_allclose(r0[k].cpu().numpy(), ref0[k].numpy(), rtol=1e-12, atol=0, err_msg=k + ' nan_to_num')
    # uint8 and int64 inputs: the same matrix
    m8, m64 = metrics.ConfusionMeter(nc, 255, device=tgt.device), metrics.ConfusionMeter(nc, 255, device=tgt.device)
    for p, t in zip(preds, gts):
        m8.update(p.to(torch.uint8), t.to(torch.uint8))
        m64.update(p, t.to(torch.uint8))
    assert torch.equal(m8.conf, meter.conf) and torch.equal(m64.conf, meter.conf)
    # merge / reset
    m8.merge(m64)
    assert torch.equal(m8.conf, 2 * meter.conf)
    assert int(m8.reset().conf.abs().sum()) == 0
    assert meter.all_reduce() is meter                  # no process group: nothing happens
    # labels that are out of range but not ignored (200): exactly intersect_and_union's areas
    gen = torch.Generator().manual_seed(SEED)
    p = torch.randint(0, nc, (37, 53), generator=gen)
    t = torch.randint(0, nc, (37, 53), generator=gen)
    t[torch.rand(37, 53, generator=gen) < 0.1] = 200
    t[torch.rand(37, 53, generator=gen) < 0.1] = 255
    odd = metrics.ConfusionMeter(nc, 255, device=tgt.device).update(p, t)
    for k, a, b in zip(('inter', 'union', 'pred', 'label'), odd.areas(), metrics.intersect_and_union(p, t, nc, 255)):
        assert torch.equal(a.cpu(), b), k
    assert int(odd.conf[nc].sum()) == int((t == 200).sum()) > 0
    # a prediction outside [0, nc) (no arg-max produces one) is dropped from every count
    wild = p.clone()
    wild[torch.rand(37, 53, generator=gen) < 0.2] = nc + 1
    kept = wild < nc
    assert torch.equal(metrics.ConfusionMeter(nc, 255, device=tgt.device).update(wild, t).conf,
                       metrics.ConfusionMeter(nc, 255, device=tgt.device).update(wild[kept], t[kept]).conf)
    # 64-bit accumulation: cells preset beyond 2^32 stay exact
    big = metrics.ConfusionMeter(nc, 255, device=tgt.device)
    big.conf.fill_(2 ** 40)
    big.update(p, t)
    assert torch.equal(big.conf - 2 ** 40, odd.conf)


def test_fused_score_equals_two_step(tgt):
    """seg_predict with gt / conf = seg_predict, then confusion_update = metrics.intersect_and_union of its labels"""
    nc, hw, out_hw, flip = 19, (44, 64), (48, 70), 1
    gen = torch.Generator().manual_seed(SEED + 7)
    lg = tgt.to(torch.randn(2, 11, 16, nc, generator=gen) * 4)
    gt = torch.randint(0, nc, (2,) + out_hw, generator=gen)
    gt[torch.rand((2,) + out_hw, generator=gen) < 0.1] = 255
    plain = ops.seg_predict(lg, hw[0], hw[1], out_hw, flip)
    two = torch.zeros(nc + 1, nc, dtype=torch.int64, device=tgt.device)
    ops.confusion_update(plain, tgt.to(gt), two, nc, 255)
    want = metrics.intersect_and_union(plain.cpu().long(), gt, nc, 255)
    for dt in (torch.uint8, torch.int64):
        conf = torch.zeros(nc + 1, nc, dtype=torch.int64, device=tgt.device)
        fused = ops.seg_predict(lg, hw[0], hw[1], out_hw, flip, tgt.to(gt.to(dt)), conf, 255)
        _sync(tgt)
        assert torch.equal(fused, plain) and torch.equal(conf, two), dt
        assert int(conf.sum()) == int((gt != 255).sum())
        meter = metrics.ConfusionMeter(nc, 255, device=tgt.device)
        meter.conf = conf
        for k, a, b in zip(('inter', 'union', 'pred', 'label'), meter.areas(), want):
            assert torch.equal(a.cpu(), b), (dt, k)
        ops.seg_predict(lg, hw[0], hw[1], out_hw, flip, tgt.to(gt.to(dt)), conf, 255)     # a second call accumulates
        assert torch.equal(conf, 2 * two), dt


def test_seg_eval_refusals(tgt):
    """every refusal is an error code without a launch: CmdaError, label_out and conf untouched"""
    nc = 19
    lg = tgt.to(torch.randn(1, 4, 4, nc))
    out = tgt.to(torch.full((1, 8, 8), 7, dtype=torch.uint8))
    conf = tgt.to(torch.full((nc + 1, nc), 3, dtype=torch.int64))
    gt = tgt.to(torch.zeros(1, 8, 8, dtype=torch.uint8))

    def raw_predict(B=1, h=4, w=4, H=8, W=8, OH=8, OW=8, nc_=nc, flip=0, gt_=None, tag=0, conf_=None):
        _lib.call('cmdax_seg_predict', ptr(lg), ptr(out), ptr(gt_), c_i32(tag), ptr(conf_), c_i32(B), c_i32(h), c_i32(w), c_i32(H),
                  c_i32(W), c_i32(OH), c_i32(OW), c_i32(nc_), c_i32(flip), c_i32(255), _lib.stream_of(lg))

    def raw_update(n=64, nc_=nc, ptag=0, gtag=0):
        _lib.call('cmdax_confusion_update', ptr(out), c_i32(ptag), ptr(gt), c_i32(gtag), ptr(conf), c_i64(n), c_i32(nc_), c_i32(255),
                  _lib.stream_of(lg))
    refused = [
        lambda: raw_predict(nc_=33), lambda: raw_predict(nc_=0),
        lambda: raw_predict(OH=46341, OW=46341),                       # B * OH * OW >= 2^31
        lambda: raw_predict(B=2, OH=32768, OW=32768),
        lambda: raw_predict(h=0), lambda: raw_predict(w=0), lambda: raw_predict(H=0), lambda: raw_predict(W=-1),
        lambda: raw_predict(OH=0), lambda: raw_predict(OW=0),
        lambda: raw_predict(flip=3), lambda: raw_predict(flip=-1),
        lambda: raw_predict(gt_=gt, tag=2, conf_=conf),                # bad dtype tag
        lambda: raw_predict(conf_=conf), lambda: raw_predict(gt_=gt),  # one of gt / conf without the other
        lambda: raw_update(nc_=33), lambda: raw_update(nc_=0), lambda: raw_update(n=-1), lambda: raw_update(ptag=5),
        lambda: raw_update(gtag=-1),
        # the same through the public functions
        lambda: ops.seg_predict(tgt.to(torch.randn(1, 4, 4, 33)), 8, 8, out=out),
        lambda: ops.seg_predict(lg, 8, 8, flip=3, out=out),
        lambda: ops.seg_predict(lg, 8, 8, conf=conf, out=out),
        lambda: ops.seg_predict(lg, 8, 8, gt=gt, out=out),
        lambda: ops.seg_predict(lg, 8, 8, gt=gt.int(), conf=conf, out=out),
        lambda: ops.seg_predict(lg, 0, 8, out_hw=(8, 8), out=out),
        lambda: ops.confusion_update(out, gt, tgt.to(torch.zeros(34, 33, dtype=torch.int64)), 33),
        lambda: ops.confusion_update(out, gt.float(), conf, nc),
    ]
    for i, f in enumerate(refused):
        with pytest.raises(CmdaError):
            f()
            pytest.fail(f'refusal {i} went through')
    _sync(tgt)
    assert bool((out == 7).all()) and bool((conf == 3).all())
    raw_predict(gt_=gt, conf_=conf)                      # (the same arguments, valid: it runs)
    _sync(tgt)
    assert int(out.max()) < nc and int(conf.sum()) == 3 * conf.numel() + 64
    # the product binding has no CPU fallback
    _lib._unbind_for_tests()
    with pytest.raises(CmdaError, match='no CPU fallback'):
        ops.seg_predict(torch.randn(1, 4, 4, nc), 8, 8)
    with pytest.raises(CmdaError, match='no CPU fallback'):
        ops.confusion_update(torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8),
                             torch.zeros(nc + 1, nc, dtype=torch.int64), nc)


# ---------------------------------------------------------------------------------------------------------------------------
# segmentors
SMALL = dict(dims=[32, 64, 160, 256], ch=64)
IN_HW = (64, 96)
METAS = [dict(ori_shape=IN_HW + (3,), flip=False),
         dict(ori_shape=(72, 100, 3), flip=True, flip_direction='horizontal'),
         dict(ori_shape=IN_HW + (3,), flip=True, flip_direction='vertical')]


def _build(kind, tgt):
    from test_fdist import make_cfg as fusion_cfg
    from test_image_uda import model_cfg
    if kind == 'fusion':
        cfg = fusion_cfg(**SMALL)['model']
    else:
        cfg = dict(model_cfg(SMALL['dims'], SMALL['ch']), type='EventsEncoderDecoder' if kind == 'events' else 'EncoderDecoder')
    model = seeded_fill(build_segmentor(cfg), 151)
    with torch.no_grad():
        model.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE)
    return model.to(tgt.device).eval()


def _memoize_network(model):
    """the network's forward pass (deterministic, and not what these tests are about) runs once per distinct input: every path
    under test -- simple_test, inference, predict -- still asks the model for it and applies its own tail"""
    def wrap(name):
        fn, memo = getattr(model, name), {}

        def cached(*args, **kw):
            key = tuple(id(a) if isinstance(a, torch.Tensor) else repr(a) for a in args + tuple(sorted(kw.items())))
            if key not in memo:
                memo[key] = (fn(*args, **kw), args, kw)     # (the arguments are kept alive: their ids stay unique)
            return memo[key][0]
        setattr(model, name, cached)
    wrap('encode_decode_lowres')
    if type(model).__name__ == 'EncoderDecoder':
        wrap('encode_decode')
    return model


def _inputs(kind, tgt, meta):
    img, ev = _input_tensors(tgt.kind)
    if kind == 'fusion':
        return dict(warp_image=img, events_vg=ev, img_metas=meta)
    if kind == 'events':
        return dict(image=img, img_metas=meta)
    return dict(img=img, img_meta=meta)


@functools.lru_cache(maxsize=None)
def _input_tensors(target_kind):
    dev = torch.device('cuda:0' if target_kind == 'gpu' else 'cpu')
    return seeded_randn((1, 3) + IN_HW, 151, 'img').to(dev), seeded_randn((1, 3) + IN_HW, 151, 'ev').clamp(-1, 1).to(dev)


def _old_scores(kind, model, kw, meta):
    """what the shipped `simple_test` takes its argmax of: `inference`'s probabilities (the plain EncoderDecoder: the logits)"""
    if kind != 'plain':
        return model.inference(True, **kw)
    return segmentors._flip_back(segmentors._resize_logits(model.encode_decode(kw['img']), meta['ori_shape']), meta)


@pytest.mark.parametrize('kind', ['fusion', 'events', 'plain'])
def test_predict_matches_simple_test(tgt, kind):
    rt.set_compute_dtype(torch.float32)
    model = _memoize_network(_build(kind, tgt))
    gen = torch.Generator().manual_seed(SEED + 11)
    for meta in METAS:
        kw = _inputs(kind, tgt, meta)
        oh, ow = meta['ori_shape'][:2]
        gt = torch.randint(0, 19, (oh, ow), generator=gen)
        gt[torch.rand(oh, ow, generator=gen) < 0.1] = 255
        with torch.no_grad():
            want = torch.from_numpy(np.stack(model.simple_test(True, **kw) if kind != 'plain' else
                                             model.simple_test(kw['img'], kw['img_meta'], True)))
            top2 = _old_scores(kind, model, kw, meta).topk(2, dim=1).values
        tie = (top2[:, 0] == top2[:, 1]).cpu()
        meter = metrics.ConfusionMeter(19, 255, device=tgt.device)
        got = model.predict(True, gt_semantic_seg=gt, meter=meter, **kw)
        assert got.dtype == torch.uint8 and got.device.type == tgt.device.type and tuple(got.shape) == (1, oh, ow) == tuple(want.shape)
        assert torch.equal(model.predict(True, **kw), got)            # (without the score: the same labels)
        check_le(f'{kind} {meta}: tied share of simple_test', tie.double().mean().item(), 1e-3)
        assert torch.equal(got.cpu().long()[~tie], want[~tie])
        res, ref = meter.compute(), metrics.mean_iou([want[0]], [gt], 19, 255)
        slack = float(tie.sum()) / float((gt != 255).sum())
        for k in NAMES:
            a, b = res[k].cpu().numpy(), ref[k].numpy()
            if slack == 0:
                np.testing.assert_allclose(a, b, rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
            elif k == 'aAcc':   # (a pixel moves the overall accuracy by at most 1 / labelled pixels)
                assert abs(float(a) - float(b)) <= slack + 1e-12
    # the UDA wrapper hands over to its student
    kw = _inputs(kind, tgt, METAS[1])
    stub = types.SimpleNamespace(get_model=lambda: model)
    meter = metrics.ConfusionMeter(19, 255, device=tgt.device)
    assert torch.equal(uda.DACS.predict(stub, True, gt_semantic_seg=torch.zeros(72, 100, dtype=torch.uint8), meter=meter, **kw), model.predict(True, **kw))
    assert int(meter.conf.sum()) == 72 * 100 and int(meter.conf[0].sum()) == 72 * 100
    # rescale=False: labels at the input size
    assert tuple(model.predict(False, **kw).shape) == (1,) + IN_HW
    saved, model.test_cfg = model.test_cfg, dict(mode='slide')
    try:
        with pytest.raises(NotImplementedError):
            model.predict(True, **kw)
    finally:
        model.test_cfg = saved


def _eval_samples(tgt):
    gen = torch.Generator().manual_seed(SEED + 13)
    out = []
    for i, meta in enumerate(METAS):
        oh, ow = meta['ori_shape'][:2]
        gt = torch.randint(0, 19, (oh, ow), generator=gen)
        gt[torch.rand(oh, ow, generator=gen) < 0.1] = 255
        out.append(dict(image=tgt.to(seeded_randn((1, 3) + IN_HW, 160 + i, 'img')), img_metas=meta, gt_semantic_seg=gt))
    return out


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype == torch.float64 and a[k].shape == b[k].shape, k
        np.testing.assert_allclose(a[k].cpu().numpy(), b[k].cpu().numpy(), rtol=1e-12, atol=0, equal_nan=True, err_msg=k)


def test_distributed_evaluate_on_device(tgt):
    """three samples with mixed flips / sizes: on_device=True returns what the default (host label maps, four bincounts per image)
    returns; alone, and on the emulator under a one-rank gloo group with the collectives forced"""
    import torch.distributed as dist
    from cmda_amd.parallel import distributed_evaluate
    rt.set_compute_dtype(torch.float32)
    model = _memoize_network(_build('events', tgt)).train()
    samples = _eval_samples(tgt)
    host = distributed_evaluate(model, samples, 19, 255)
    dev = distributed_evaluate(model, samples, 19, 255, on_device=True)
    assert model.training                                # the caller's state is restored
    _same(dev, host)
    assert bool(torch.isnan(host['IoU']).any()) == bool(torch.isnan(dev['IoU']).any())
    _same(distributed_evaluate(model, samples, 19, 255, nan_to_num=0, on_device=True), distributed_evaluate(model, samples, 19, 255, nan_to_num=0))
    with pytest.raises(ValueError):
        distributed_evaluate(model, samples, 19, 255, label_map={5: 4}, on_device=True)
    with pytest.raises(ValueError):
        distributed_evaluate(model, samples, 19, 255, reduce_zero_label=True, on_device=True)
    if tgt.kind != 'emu':
        return
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1')
    dist.init_process_group('gloo', rank=0, world_size=1)
    try:
        _same(distributed_evaluate(model, samples, 19, 255, force=True, on_device=True), host)
        empty = distributed_evaluate(model, [], 19, 255, force=True, on_device=True)
        assert empty['IoU'].shape == (19,) and bool(torch.isnan(empty['IoU']).all())
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_predict_against_reference_gpu():
    """tests/golden/image_simple_test.npz: the reference's own EventsEncoderDecoder.simple_test at 440 x 640 (the model and the
    bound of test_image_uda.py::test_simple_test_against_reference_gpu)"""
    from test_image_uda import SEEDS, _gpu, golden, model_cfg
    _gpu()
    g = golden('image_simple_test.npz')
    rt.set_compute_dtype(torch.float32)
    m = build_segmentor(model_cfg(DACS_DIMS, DACS_CH))
    seeded_fill(m, SEEDS['simple'])
    with torch.no_grad():
        m.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE)
    m = m.cuda().eval()
    img = seeded_randn((1, 3, 440, 640), SEEDS['simple'], 'img').cuda()
    for key in ('image', 'warp_image'):
        for flip in (False, True):
            meta = dict(ori_shape=(440, 640, 3), flip=flip, flip_direction='horizontal')
            seg = m.predict(True, **{key: img, 'img_metas': meta})
            assert seg.dtype == torch.uint8 and seg.is_cuda and tuple(seg.shape) == (1, 440, 640)
            seg = seg.cpu().numpy()[..., ::4, ::4]   # (the fixture keeps every fourth row / column)
            ref = g[f'{key}.flip{int(flip)}'].numpy()
            check_le(f'predict {key} flip={flip}: label disagreement', 1 - (seg == ref).mean(), 1e-3)
