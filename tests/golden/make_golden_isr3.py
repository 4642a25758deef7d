"""Generates tests/golden/isr3.npz from the reference's OWN get_image_change_from_pil and cow_masks (mmseg/datasets/utils.py:108-152,
:155-200), imported unmodified through ref_shim:
  * a 48 x 72 uint8 RGB image (6 x 6 blocks plus noise) and, for each of the five three-channel presets (cityscapes_ic.py:101-110,
    dark_zurich_ic.py:112-121, dacs.py:162-165), the [3,48,72] result of the reference's loop over get_image_change_from_pil;
  * for two seeds at 100 x 132: the np.random.normal field cow_masks drew (as the fp32 it casts it to), p and sigma as the reference
    drew them (recorded from its own torch calls), the next torch.rand(1) after the call, and the mask it returned for the loader's
    arguments (cityscapes_ic.py:264-265).
The preset tables are typed here from the cited lines as data; only arrays go into the file.  Runs only in the authoring container.
Usage: python tests/golden/make_golden_isr3.py
"""
import math
import os
import sys

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

H, W = 48, 72
CH, CW = 100, 132
COW_SEEDS = (0, 1)
# (val_range, [(threshold, clip_range, shift_pixel)] x 3)
PRESETS = {
    'day': ((1, 10), [(0.025, 0.05, 1), (0.030, 0.20, 3), (0.040, 0.32, 5)]),
    'new_day': ((1e-5, 255 + 1e-5), [(0, 0.015, 1), (0, 0.040, 3), (0, 0.070, 5)]),
    'night': ((9, 255 + 9), [(0.012, 0.04, 1), (0.012, 0.12, 3), (0.012, 0.20, 5)]),
    'new_night': ((500, 1000), [(0.015, 0.05, 1), (0.02, 0.12, 3), (0.025, 0.2, 5)]),
    'dacs': ((9, 255 + 9), [(0.012, 0.04, 1), (0.012, 0.12, 3), (0.012, 0.20, 5)]),
}


def image():
    g = torch.Generator().manual_seed(31)
    base = torch.rand((H // 6, W // 6, 3), generator=g).repeat_interleave(6, 0).repeat_interleave(6, 1)
    return ((base * 0.8 + 0.2 * torch.rand((H, W, 3), generator=g)) * 255).to(torch.uint8).numpy()


def main():
    ut = ref_shim.load('mmseg.datasets.utils')
    rgb = image()
    pil = Image.fromarray(rgb)
    out = dict(rgb=rgb, cow_seeds=np.array(COW_SEEDS))
    for name, (val_range, rows) in PRESETS.items():
        chans = [ut.get_image_change_from_pil(pil, width=W, height=H, val_range=val_range, _threshold=t, _clip_range=c, shift_pixel=s)
                 for t, c, s in rows]
        out[f'isr_{name}'] = torch.cat(chans, dim=0).numpy()
        assert out[f'isr_{name}'].shape == (3, H, W)
    saved_normal, saved_uniform = np.random.normal, torch.Tensor.uniform_
    for s in COW_SEEDS:
        fields, draws = [], []

        def normal(*a, **k):
            r = saved_normal(*a, **k)
            fields.append(r.copy())
            return r

        def uniform_(t, *a, **k):
            r = saved_uniform(t, *a, **k)
            draws.append(r.clone())
            return r
        torch.manual_seed(s)
        np.random.seed(s)
        np.random.normal, torch.Tensor.uniform_ = normal, uniform_
        try:
            mask = ut.cow_masks(torch.zeros([1, 1, CH, CW]), prop_range=[0.7, 0.7], log_sigma_range=[math.log(16), math.log(17)])
        finally:
            np.random.normal, torch.Tensor.uniform_ = saved_normal, saved_uniform
        nxt = torch.rand(1)
        assert len(fields) == 1 and len(draws) == 2
        out.update({f'cow{s}_field': fields[0][0, 0].astype(np.float32), f'cow{s}_p': draws[0].numpy(),
                    f'cow{s}_sigma': torch.exp(draws[1]).numpy(), f'cow{s}_next_rand': nxt.numpy(),
                    f'cow{s}_mask': mask[0, 0].numpy().astype(np.uint8)})
        print(f'cow seed {s}: p {float(draws[0]):.6f} sigma {float(torch.exp(draws[1])):.6f} kept {float(mask.float().mean()):.4f}')
    path = os.path.join(HERE, 'isr3.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
