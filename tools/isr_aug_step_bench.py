"""ms per training step of BASELINE.json configs[3] (bench.py's workload: full CMDA UDA step, MiT-B5, 512 x 512, 2 + 2 samples, bf16,
hipGraph replay, overlapped optimizer update) with the ISR augmentations off and on (sky_mask = a 4-image uint8 bank,
isr_noise_dacs_type = 'noise+blur').  bench.py itself stays augmentation-off; this tool only reuses its config and data.
Runs alternate off / on `--rounds` times in one process; prints one JSON line.
With `--isr3` the pair is instead the same step as train type 'cs2dz_image+raw-isr' (AttentionFusion, no generator: the train type the
reference's three-channel launch uses) with uda.shift_3_channel off and on; off is the one-channel mixed ISR.

    python tools/isr_aug_step_bench.py --steps 30 --warmup 5 --rounds 2 [--isr3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402


def dz_cfg(shift_3_channel):
    cfg = bench.dacs_cfg()
    tt = 'cs2dz_image+raw-isr'
    cfg['model'].update(train_type=tt, fusion_module=dict(cfg['model']['fusion_module'], type='AttentionFusion'))
    cfg['model']['decode_head']['decoder_params']['train_type'] = tt
    cfg['uda'].update(train_type=tt, cyclegan_itrd2en_path='')
    if shift_3_channel:
        cfg['uda'].update(shift_3_channel=True, isr_parms='')
    return cfg


def run(on, steps, warmup, dev, isr3=False):
    import cmda_amd.runtime as rt
    from cmda_amd import optim
    from cmda_amd.registry import build_train_model
    rt.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(1234)
    cfg = dz_cfg(on) if isr3 else bench.dacs_cfg()
    if on and not isr3:
        bank = torch.randint(0, 256, (4, 512, 512), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
        cfg['uda'].update(sky_mask=bank, isr_noise_dacs_type='noise+blur')
    dacs = build_train_model(cfg)
    dacs.init_weights()
    dacs.to(dev).train()
    opt = optim.FlatAdamW(dacs.model, lr=6e-5, weight_decay=0.01, custom_keys=bench.CUSTOM_KEYS)
    opt.overlap = True
    dacs.attach_flat_store(opt)
    batch = bench.synthetic_pairs(2, 512, 100, dev)
    torch.manual_seed(1000)
    np.random.seed(1000)
    dacs.enable_graph(warmup_iters=2)
    it = [0]

    def step():
        opt.zero_grad()
        lv = dacs(**batch)
        opt.step(optim.poly_warm_scale(it[0]))
        it[0] += 1
        return lv

    for _ in range(3 + warmup):
        step()
    opt.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        lv = step()
    opt.synchronize()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    assert dacs._graph is not None
    out = dict(ms_per_step=round(ms, 3), losses={k: round(float(v), 5) for k, v in lv.items() if 'loss' in k})
    if on and not isr3:
        out['sky_pixels'] = [int((batch['source']['label'][b] == 10).sum()) for b in range(2)]
    del dacs, opt
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--isr3', action='store_true', help="time 'cs2dz_image+raw-isr' with uda.shift_3_channel off / on instead")
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    runs = {'off': [], 'on': []}
    for _ in range(args.rounds):
        runs['off'].append(run(False, args.steps, args.warmup, dev, args.isr3))
        runs['on'].append(run(True, args.steps, args.warmup, dev, args.isr3))
    off = [r['ms_per_step'] for r in runs['off']]
    on = [r['ms_per_step'] for r in runs['on']]
    if args.isr3:
        print(json.dumps(dict(workload="BASELINE.json configs[3] as 'cs2dz_image+raw-isr', bf16, hipGraph replay", steps=args.steps,
                              warmup=args.warmup, shift_3_channel_off_ms=off, shift_3_channel_on_ms=on,
                              shift_3_channel_cost_ms=round(min(on) - min(off), 3), runs=runs)))
        return
    print(json.dumps(dict(workload='BASELINE.json configs[3], bf16, hipGraph replay', steps=args.steps, warmup=args.warmup,
                          aug_off_ms=off, aug_on_ms=on, aug_cost_ms=round(min(on) - min(off), 3), runs=runs)))


if __name__ == '__main__':
    main()
