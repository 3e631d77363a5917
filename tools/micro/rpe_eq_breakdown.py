"""What the equivariant RPE logits kernel pays over the invariant one, at the bench shape (16 clouds per launch): the kernel as it is,
and without the equivariant term (same 24 folded-query rows, no eq-embedding reads).  (The other rows of profiles/r0[456]_rpe_eq_breakdown.txt
-- logits written over one block, other workgroup counts, the round-3 request order -- came from tuning hooks that are gone.)
python tools/micro/rpe_eq_breakdown.py"""
import os, sys; R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, 'tools'))
import time, torch
import bench_attention_stack as B
x = torch.randn(4096, 4096, device='cuda'); t0 = time.time()
while time.time() - t0 < 1.5: y = x @ x
torch.cuda.synchronize()
lengths = (382, 350, 304, 310, 382, 350, 304, 310, 382, 350, 304, 310, 382, 350, 304, 310)
emb_gb = sum(n * n for n in lengths) * 256 * 4 / 1e9
for A, eq in ((1, False), (6, True)):
    B.run(A, lengths[:2], eq, iters=1, check=True)
for rep in range(2):
    for name, A, eq in (('A=6 eq (default)', 6, True), ('A=6 without the eq term', 6, False), ('A=1 invariant', 1, False)):
        tb, ta, nbytes = B.run(A, lengths, eq, iters=20)
        print('%-40s logits kernel %6.1f us  (embedding stream alone %.2f GB -> %.2f TB/s)   attention %6.1f us' % (name, tb, emb_gb, emb_gb / tb * 1e3, ta))
