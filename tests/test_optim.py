"""Flat AdamW vs torch.optim.AdamW with the reference's paramwise rules; schedule vs the oracle restatement."""
import pytest
import torch

from cmda_amd import ops, optim
from conftest import assert_close
from oracle import uda as ouda


def test_flat_adamw_matches_torch(tgt):
    torch.manual_seed(0)
    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.norm1 = torch.nn.LayerNorm(10)
            self.fc = torch.nn.Linear(10, 7)
            self.decode_head = torch.nn.Linear(7, 5)
    net, ref = Net().to(tgt.device), Net()
    ref.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    keys = dict(head=dict(lr_mult=10.0), pos_block=dict(decay_mult=0.0), norm=dict(decay_mult=0.0))
    opt = optim.FlatAdamW(net, lr=1e-3, weight_decay=0.01, custom_keys=keys)
    groups = []
    for n, p in ref.named_parameters():
        lr, wd = ouda.param_group_options(n, 1e-3, 0.01, keys)
        groups.append(dict(params=[p], lr=lr, weight_decay=wd))
    topt = torch.optim.AdamW(groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    for it in range(3):
        opt.zero_grad()
        for (n, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
            g = torch.randn(q.shape)
            q.grad = g.clone()
            p.grad.copy_(g)
        opt.step()
        topt.step()
    for (n, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        # three fused steps against torch.optim.AdamW: fp32 round-off of a handful of operations per element (1e-6 of the tensor's
        # largest element measured on the MI355X; the absolute term covers a near-zero bias whose whole range is 3e-3)
        assert_close(p.data, q.data, 2e-6, atol=5e-9, name=n)


# The parameter-state streams (cmda_ema_update, cmda_adamw_step) run ceil(n / 2048) blocks of 256 threads, capped at 1024
# (CMDA_STREAM_BLOCKS), two 16-byte vectors per thread and loop pass.  n = 6 000 003: the capped grid (a pass covers 1024 x 256 x 8
# elements), so every thread takes its second vector, most a second loop iteration, and the ragged tail of 3 runs.
# n = 2048 k + 3: k + 1 blocks, the last of them nearly empty.
_STREAM_N = [6000003, 2048 + 3, 2 * 2048 + 3, 3 * 2048 + 3]


@pytest.mark.parametrize('mirror', [False, True], ids=['nomirror', 'bf16mirror'])
@pytest.mark.parametrize('n', _STREAM_N)
def test_ema_update_stream(tgt, n, mirror):
    torch.manual_seed(n)
    p, e = torch.randn(n), torch.randn(n)
    ed = tgt.to(e.clone())
    md = torch.full((n,), float('nan'), dtype=torch.bfloat16, device=tgt.device) if mirror else None
    ops.ema_update(ed, tgt.to(p), 0.999, mirror=md)
    ref = 0.999 * e.double() + (1 - 0.999) * p.double()
    assert_close(ed, ref, 1e-6, name='ema')                       # (the bound of test_classmix_ema_adamw)
    if mirror:
        assert_close(md, ref, 4e-3, name='ema bf16 mirror')     # one rounding of the fp32 result: <= 2^-8 of the largest element
        assert torch.equal(md.cpu(), ed.cpu().bfloat16()), 'the mirror is the rounded fp32 result'


@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'off16'])
@pytest.mark.parametrize('n', _STREAM_N)
def test_adamw_step_stream(tgt, n, offset):
    """three steps against torch.optim.AdamW; offset 1: every tensor sliced one element off 16-byte alignment (the entry point falls
    back to the scalar kernel there)"""
    torch.manual_seed(n + offset)
    prm = torch.nn.Parameter(torch.randn(n))
    opt = torch.optim.AdamW([prm], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)

    def buf(src=None, dtype=torch.float32):
        t = torch.zeros(n + offset, dtype=dtype, device=tgt.device)[offset:]
        if src is not None:
            t.copy_(src)
        return t
    pd, m, v, pb = buf(prm.data), buf(), buf(), buf(dtype=torch.bfloat16)
    assert (pd.data_ptr() % 16 == 0) == (offset == 0)
    for step in (1, 2, 3):
        gr = torch.randn(n)
        prm.grad = gr.clone()
        opt.step()
        ops.adamw_step(pd, buf(gr), m, v, 1e-2, 0.9, 0.999, 1e-8, 0.01, step, p_bf16=pb)
    assert_close(pd, prm.data, 2e-6, name='adamw')                  # (the bounds of test_classmix_ema_adamw)
    assert_close(pb, prm.data, 4e-3, name='adamw bf16 copy')
    assert torch.equal(pb.cpu(), pd.cpu().bfloat16()), 'the bf16 copy is the rounded fp32 master'
    st = opt.state[prm]
    assert_close(m, st['exp_avg'], 2e-6, name='adamw exp_avg')
    # the kernel forms 1 - beta2 from the fp32 beta2 (consistent with its bias correction, so p agrees to 2e-6), torch rounds the
    # double 1 - 0.999: the two factors differ by up to half an ulp of beta2 over 1 - beta2, 2^-25 / 1e-3 = 3e-5 (1.3e-5 here)
    assert_close(v, st['exp_avg_sq'], 2e-6 + 2.0 ** -25 / (1 - 0.999), name='adamw exp_avg_sq')


def test_schedule_matches_oracle():
    for it in (0, 1, 700, 1499, 1500, 20000, 39999):
        assert abs(optim.poly_warm_scale(it) * 6e-5 - ouda.poly_warm_lr(6e-5, it)) < 1e-15
