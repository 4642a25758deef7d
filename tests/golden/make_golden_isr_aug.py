"""Generates tests/golden/isr_aug.npz from the reference's OWN sky_mask_transform and add_noise_on_isr
(mmseg/models/utils/dacs_transforms.py:134-171, :186-211), imported unmodified through ref_shim (Tensor.cuda is the identity there):
for two seeds at 64 x 96 the inputs, a two-image noise bank (written as PNG files, read back by the reference through PIL), the
decisions the reference drew (recorded from its own torch calls, not re-derived), the three CPU randn_like fields and the outputs.
Only arrays go into the file.  Runs only in the authoring container.
Usage: python tests/golden/make_golden_isr_aug.py
"""
import os
import sys
import tempfile

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

H, W = 64, 96
SEEDS = (3, 4)   # (the blur coin of add_noise_on_isr falls once on either side)


class Recorder:
    """wraps the torch entry points the two functions draw from and keeps what they returned, in call order"""
    NAMES = ('randint', 'randperm', 'rand', 'randn_like')

    def __enter__(self):
        self.log = []
        self.saved = {n: getattr(torch, n) for n in self.NAMES}
        self.uniform_ = torch.Tensor.uniform_
        for n in self.NAMES:
            setattr(torch, n, self.wrap(n, self.saved[n]))
        rec = self

        def uniform_(t, *a, **k):
            r = rec.uniform_(t, *a, **k)
            rec.log.append(('uniform_', r.clone()))
            return r
        torch.Tensor.uniform_ = uniform_
        return self

    def wrap(self, name, fn):
        def w(*a, **k):
            r = fn(*a, **k)
            self.log.append((name, r.clone()))
            return r
        return w

    def __exit__(self, *exc):
        for n in self.NAMES:
            setattr(torch, n, self.saved[n])
        torch.Tensor.uniform_ = self.uniform_

    def of(self, name):
        return [v for n, v in self.log if n == name]


def inputs(seed):
    g = torch.Generator().manual_seed(1000 + seed)
    isr = torch.rand(1, H, W, generator=g) * 2 - 1
    label = torch.randint(0, 19, (1, H, W), generator=g)
    label[label == 10] = 11
    if seed == SEEDS[0]:
        label[0, :20, 30:] = 10          # a sky region on two borders
    else:
        label[0, 24:40, 16:50] = 10      # an interior blob
        label[0, 50, 60:90] = 10         # and a thin stripe
    return isr, label


def main():
    dt = ref_shim.load('mmseg.models.utils.dacs_transforms')
    g = torch.Generator().manual_seed(77)
    bank = torch.randint(0, 256, (2, H, W), generator=g, dtype=torch.uint8)
    out = dict(bank=bank.numpy(), seeds=np.array(SEEDS))
    with tempfile.TemporaryDirectory() as tmp:
        names = ['n0.png', 'n1.png']
        for n, img in zip(names, bank):
            Image.fromarray(img.numpy()).save(os.path.join(tmp, n))
        param = dict(noise_root_path=tmp + '/', noise_list=names)
        for s in SEEDS:
            isr, label = inputs(s)
            torch.manual_seed(s)
            with Recorder() as r:
                sky = dt.sky_mask_transform(param, isr.clone(), label)
            ri, ru, rp = r.of('randint'), r.of('uniform_'), r.of('randperm')
            assert len(ri) == 2 and len(ru) == 2 and len(rp) == 2
            torch.manual_seed(s)
            with Recorder() as r:
                noisy = dt.add_noise_on_isr(isr.clone(), transform_type='noise+blur')
            coin, nu, nf = r.of('rand'), r.of('uniform_'), r.of('randn_like')
            assert len(coin) == 1 and len(nu) == 3 and len(nf) == 3
            out.update({f's{s}_isr': isr.numpy(), f's{s}_label': label.numpy().astype(np.uint8),
                        f's{s}_sky_k_drawn': ri[0].numpy(), f's{s}_sky_lambda': ru[0].numpy(), f's{s}_sky_intensity': ru[1].numpy(),
                        f's{s}_sky_index': ri[1].numpy(), f's{s}_sky_row_perm': rp[0].numpy(), f's{s}_sky_col_perm': rp[1].numpy(),
                        f's{s}_sky_out': sky.numpy(),
                        f's{s}_noise_blur': np.array(int(bool(coin[0] < 0.5))), f's{s}_noise_t1': nu[0].numpy(),
                        f's{s}_noise_t2': nu[1].numpy(), f's{s}_noise_intensity': nu[2].numpy(),
                        f's{s}_noise_fields': torch.stack(nf).numpy(), f's{s}_noise_out': noisy.numpy()})
            print(f'seed {s}: k drawn {int(ri[0])}, bank {int(ri[1])}, blur {int(bool(coin[0] < 0.5))}, sky pixels {int((label == 10).sum())}')
    path = os.path.join(HERE, 'isr_aug.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
