"""Generates tta.npz from the reference's OWN code (imported unmodified through ref_shim, with make_golden's helpers): the plain
EncoderDecoder (mmseg/models/segmentors/encoder_decoder.py:19-304) of the image_simple_test case -- the same reduced-width model,
model seed and DACS_SEG_SCALE, a 1 x 3 x 440 x 640 input of seed IMG_SEED -- under test_cfg = dict(mode='slide', crop_size=(256, 256), stride=(192, 192)):
`simple_test` with the flip off and on, and `aug_test` over three views {440 x 640; 440 x 640 flipped; 330 x 480}.  Stored per run:
every fourth row / column of the label map (uint8) and of the mask of pixels whose top-2 gap of the final score (the output of
`inference`, averaged over the views for aug_test) is below 1e-3 of the top score.  Runs only in the authoring container.
Usage: python tests/golden/make_golden_tta.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import ref_shim  # noqa: E402
from make_golden_image import SEEDS, image_model_cfg  # noqa: E402
from weights import DACS_SEG_SCALE, seeded_fill, seeded_randn  # noqa: E402

SLIDE = dict(mode='slide', crop_size=(256, 256), stride=(192, 192))
ORI = (440, 640, 3)
GAP = 1e-3
IMG_SEED = 142   # (the case's own input seed, 141, leaves 1.3e-3 of the aug_test pixels within GAP: above the 1e-3 this file asserts)


def views(img):
    """the inputs and metas of the multi-view run: scale 1.0, scale 1.0 flipped, 0.75 (330 x 480)"""
    small = F.interpolate(img, size=(330, 480), mode='bilinear', align_corners=False)
    return ([img, img.flip(dims=(3,)).contiguous(), small],
            [dict(ori_shape=ORI, flip=False), dict(ori_shape=ORI, flip=True, flip_direction='horizontal'), dict(ori_shape=ORI, flip=False)])


def near_mask(score):
    top2 = score.topk(2, dim=1).values
    return ((top2[:, 0] - top2[:, 1]) < GAP * top2[:, 0]).to(torch.uint8)


def tta():
    nn.Module.cuda = lambda self, *a, **k: self
    mm = sys.modules['mmseg.models']
    for k in ('BaseSegmentor', 'BaseSegmentorEvents', 'BaseSegmentorFusion'):
        setattr(mm, k, getattr(mg.ns.seg_base, k))
    S = ref_shim.load('mmseg.models.segmentors.encoder_decoder')

    class _Cfg(dict):   # (mmcv's ConfigDict: slide_inference reads test_cfg.stride / .crop_size)
        __getattr__ = dict.__getitem__
    cfg = image_model_cfg()
    cfg.pop('type')
    cfg['test_cfg'] = _Cfg(SLIDE)
    m = S.EncoderDecoder(**cfg)
    seeded_fill(m, SEEDS['simple'])
    with torch.no_grad():
        m.decode_head.conv_seg.weight.mul_(DACS_SEG_SCALE)
    m.eval()
    img = seeded_randn((1, 3, 440, 640), IMG_SEED, 'img')
    out = {}
    with torch.no_grad():
        for flip in (False, True):
            meta = [dict(ori_shape=ORI, flip=flip, flip_direction='horizontal')]
            seg = np.stack(m.simple_test(img, meta, True))
            score = m.inference(img, meta, True)
            assert np.array_equal(seg, score.argmax(dim=1).numpy())
            out[f'slide.flip{int(flip)}'], out[f'mask.slide.flip{int(flip)}'] = seg, near_mask(score).numpy()
        imgs, metas = views(img)
        seg = np.stack(m.aug_test(imgs, [[mt] for mt in metas], True))
        score = sum(m.inference(i, [mt], True) for i, mt in zip(imgs, metas)) / len(imgs)
        out['aug'], out['mask.aug'] = seg, near_mask(score).numpy()
        assert float((seg != score.argmax(dim=1).numpy()).mean()) <= 1e-5   # (the same sum up to its order)
    for k in list(out):
        assert out[k].shape == (1, 440, 640), (k, out[k].shape)
        out[k] = out[k].astype(np.uint8)[..., ::4, ::4]
    for k in out:
        if k.startswith('mask.'):
            share = float(out[k].mean())
            print(k, 'masked share', share)
            assert share <= 1e-3, f'{k}: {share} of the pixels are near-ties; pick another seed'
    mg.save('tta', **out)


if __name__ == '__main__':
    tta()
