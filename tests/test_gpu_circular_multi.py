"""Circular products on several GPUs (include/kdehip.h sections 2 and 2b: kdehip_prod_philox_manifold,
kdehip_product_multi_create_manifold), run on ONE GPU with KDEHIP_ALIAS_DEVICES=1 in a fresh child process, as
tests/test_gpu_multi.py runs the Euclidean multi-device paths: the result must not depend on the number of devices."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_SCRIPT = r'''
import numpy as np, torch, kdehip
from tests.circular_plan_cases import assert_points, cut_trees, oracle_run
D, Ns, Np, Niter, circ, seed = 3, [90, 70, 80], 101, 2, [1, 0, 1], 77
M = len(Ns)
g, o = cut_trees(21, D, Ns, circ)
one = kdehip.prodAppxMSGibbsS(None, g, None, None, Niter=Niter, Np=Np, seed=seed, manifold=circ, fast_circular=True)
for G in (2, 3):
    many = kdehip.prodAppxMSGibbsS(None, g, None, None, Niter=Niter, Np=Np, seed=seed, manifold=circ, ngpus=G)
    assert np.array_equal(one[0], many[0]) and np.array_equal(one[1], many[1]), G
# ... which is the plan's result, and the oracle's labels
with kdehip.ProductPlan(g, manifold=circ) as plan:
    pp, pi = plan.sample(Np, Niter=Niter, seed=seed)
assert np.array_equal(pp, one[0]) and np.array_equal(pi, one[1])
op, oi, _ = oracle_run(o, Ns, D, Np, Niter, circ, seed)
assert np.array_equal(pi, oi)
assert_points(pp, op, circ, "kdehip_prod_philox_manifold")
# the front door on one GPU keeps its route (the generic arithmetic on the host twin of the streams): same labels
slow = kdehip.prodAppxMSGibbsS(None, g, None, None, Niter=Niter, Np=Np, seed=seed, manifold=circ)
assert np.array_equal(slow[1], one[1])
assert_points(slow[0], one[0], circ, "front door, one GPU")
# a label trace over three logical devices
glbs = kdehip.makeEmptyGbGlb(recordChoosen=True)
kdehip.prodAppxMSGibbsS(None, g, None, None, Niter=Niter, Np=Np, seed=seed, manifold=circ, ngpus=3, glbs=glbs)
with kdehip.ProductPlan(g, manifold=circ) as plan:
    lab = plan.sample(Np, Niter=Niter, seed=seed, want_labels=True)[2]
L = lab.shape[2]
assert all(glbs.labelsChoosen[s + 1][j + 1][l + 1] == lab[s, j, l] for s in range(Np) for j in range(M) for l in range(L))
# resident multi plans: every device's arrays hold the complete single-plan result
dev = torch.device("cuda", 0)
with kdehip.MultiProductPlan(g, first_device=0, ngpus=2) as emp:
    Ps = [torch.zeros(D * Np, dtype=torch.float64, device=dev) for _ in range(2)]
    Is = [torch.zeros(M * Np, dtype=torch.int64, device=dev) for _ in range(2)]
    emp.sample_philox_device(Np, Niter, seed, 0, True, Ps, Is)
    torch.cuda.synchronize()
    euclid_transfers = emp.transfers_per_product
with kdehip.MultiProductPlan(g, first_device=0, ngpus=2, manifold=circ) as mp:
    assert mp.ngpus == 2 and list(mp.manifold) == circ
    Ps = [torch.zeros(D * Np, dtype=torch.float64, device=dev) for _ in range(2)]
    Is = [torch.zeros(M * Np, dtype=torch.int64, device=dev) for _ in range(2)]
    sts = [torch.cuda.Stream(device=dev) for _ in range(2)]
    mp.sample_philox_device(Np, Niter, seed, 0, True, Ps, Is, [s.cuda_stream for s in sts])
    for s in sts:
        s.synchronize()
    torch.cuda.synchronize()
    assert mp.transfers_per_product == euclid_transfers
    for k in range(2):
        assert np.array_equal(Ps[k].cpu().numpy().reshape(Np, D).T, pp), k
        assert np.array_equal(Is[k].cpu().numpy().reshape(Np, M).T, pi), k
print("circular alias ok")
'''


def test_circular_products_on_aliased_devices():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, KDEHIP_ALIAS_DEVICES="1", PYTHONPATH=root)
    out = subprocess.run([sys.executable, "-c", _SCRIPT], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "circular alias ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
