"""Generates tests/golden/ohem.npz from the reference's OWN OHEMPixelSampler.sample (mmseg/core/seg/sampler/ohem_pixel_sampler.py:32-78,
imported unmodified through ref_shim) on the CPU: seeded logits [2,19,24,32] at the labels' resolution, labels with about 5 % of 255,
and the weight maps of five settings -- one per regime of the sampler.  The generator asserts that each setting is in the regime it is
named for.  The context is a stand-in for the decode head: its ignore_index and the reference's own CrossEntropyLoss (the loss the
`thresh=None` mode sorts).  Only arrays go into the file.  Runs only in the authoring container.
Usage: python tests/golden/make_golden_ohem.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

B, NC, H, W = 2, 19, 24, 32
SEED = 171
# name -> (thresh, min_kept)
SETTINGS = {'thresh_wins': (0.7, 2), 'kth_wins': (0.05, 500), 'kth_last': (0.7, 100000), 'loss_300': (None, 300), 'loss_all': (None, 100000)}


def inputs():
    """the label's class gets + 2 on logits of scale 3: its probability spreads over (0, 1), about a third below 0.05"""
    g = torch.Generator().manual_seed(SEED)
    label = torch.randint(0, NC, (B, 1, H, W), generator=g)
    logits = torch.randn(B, NC, H, W, generator=g) * 3
    logits.scatter_add_(1, label, torch.full((B, 1, H, W), 2.0))
    label[torch.rand(B, 1, H, W, generator=g) < 0.05] = 255
    return logits, label


def main():
    ns = ref_shim.load_hotpath()
    sampler_mod = ref_shim.load('mmseg.core.seg.sampler.ohem_pixel_sampler')
    context = types.SimpleNamespace(ignore_index=255, loss_decode=ns.ce.CrossEntropyLoss(use_sigmoid=False, loss_weight=1.0))
    logits, label = inputs()
    valid = label[:, 0] != 255
    n_valid = int(valid.sum())
    prob = logits.softmax(1).gather(1, label.clamp(max=NC - 1))[:, 0][valid].sort()[0]
    assert 0.03 < 1 - n_valid / valid.numel() < 0.07
    out = dict(logits=logits.numpy(), label=label.numpy().astype(np.uint8))
    for name, (thresh, min_kept) in SETTINGS.items():
        sampler = sampler_mod.OHEMPixelSampler(context, thresh=thresh, min_kept=min_kept)
        wt = sampler.sample(logits, label)
        assert wt.shape == (B, H, W) and bool(((wt == 0) | (wt == 1)).all()) and not bool(wt[~valid].any())
        out['weight.' + name] = wt.numpy().astype(np.uint8)
        print(f'{name}: thresh {thresh}, min_kept {min_kept}: {int(wt.sum())} of {n_valid} valid pixels')
    kept = {k: int(out['weight.' + k].sum()) for k in SETTINGS}
    # the regimes
    assert prob[2 * B] < 0.7 and kept['thresh_wins'] == int((prob < 0.7).sum()), 'thresh wins'
    assert 500 * B < n_valid - 1 and prob[500 * B] > 0.05 and kept['kth_wins'] == 500 * B, 'the order statistic wins'
    assert prob[-1] > 0.7 and kept['kth_last'] == int((prob < prob[-1]).sum()) >= n_valid - 2, 'k = n_valid - 1'
    assert kept['loss_300'] == 300 * B and kept['loss_all'] == n_valid
    np.savez_compressed(os.path.join(HERE, 'ohem.npz'), **out)
    print('wrote ohem.npz', os.path.getsize(os.path.join(HERE, 'ohem.npz')), 'bytes')


if __name__ == '__main__':
    main()
