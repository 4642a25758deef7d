"""graph-timed (dependent launches replayed from a hipGraph) fused attention kernels at the encoder's stage shapes"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from cmda_amd import ops


def timeit(fn, iters=40, reps=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(iters):
                fn()
        g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (iters * reps) * 1e3


# usage: attn_graph_bench.py [batches, default 4,2] [dtype, default bf16] [keys, default 256] -- e.g. 2,4,8 when the queries-per-block rule is
# re-measured; fp32 times the split-bf16 instances (q / kv / dO / direct dK|dV in fp32; 128 queries per block from 256 blocks of 128 up,
# AttnSplit::block_switch in attention.hip, restated below); keys < 256 times the masked bf16 instances instead of the full-key ones
batches = [int(x) for x in sys.argv[1].split(',')] if len(sys.argv) > 1 else [4, 2]
dt = {'bf16': torch.bfloat16, 'fp32': torch.float32}[sys.argv[2] if len(sys.argv) > 2 else 'bf16']
Nk = int(sys.argv[3]) if len(sys.argv) > 3 else 256
for (B, N, heads) in [(B, N, heads) for (N, heads) in ((16384, 1), (4096, 2), (1024, 5), (256, 8)) for B in batches]:
    C = heads * 64
    q = torch.randn(B * N, C, device='cuda').to(dt); kv = torch.randn(B * Nk, 2 * C, device='cuda').to(dt); do = torch.randn_like(q)
    direct = ops.attention_bwd_direct(B, N, Nk, heads)
    dkv32 = None if direct else torch.zeros(B * Nk, 2 * C, device='cuda')
    dkv16 = torch.empty(B * Nk, 2 * C, device='cuda', dtype=dt) if direct else None
    o = torch.empty_like(q)
    tf = timeit(lambda: ops.attention_fused_fwd(q, kv, B, N, Nk, heads, C, 0.125))
    tb = timeit(lambda: ops.attention_fused_bwd(q, kv, do, dkv32, B, N, Nk, heads, C, 0.125, dkv16=dkv16))
    qpb = ops.attention_fwd_queries_per_block(B, N, heads, Nk=Nk) if dt == torch.bfloat16 else (64 if -(-N // 128) * heads * B < 256 else 128)
    print(f'B{B} N{N} heads{heads}: fwd {tf:6.1f} us   bwd (dq + dkv) {tb:6.1f} us  direct={direct}  queries/block={qpb}', flush=True)
