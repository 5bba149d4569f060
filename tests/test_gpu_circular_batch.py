"""Circular products in BATCHED launches (include/kdehip.h section 2e: kdehip_prod_philox_batch_manifold, the batched
sampling instantiation of the general kernel's circular fast mode, 8 chains per workgroup): every item of a batch must be
byte for byte the single `prodAppxMSGibbsS_device(manifold=)` call -- whichever launch it rides, whatever its position --
and `mul_device_batch(manifold=)`, which samples through the same path, byte for byte `mul_device(manifold=)`.
Chain counts are no multiples of the workgroup width, so the dead chains of a product's last workgroup are exercised.
Byte equality alone would also hold if every circular item fell back to the one-by-one route, so the tests read which route
each call took (`kdehip.batch_launches()`: batched launches and items enqueued singly), and one item carries `d_labels`:
the label trace stored by the batched build must be the single call's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kdehip
from tests.circular_plan_cases import cut_trees, refused_trees

pytestmark = pytest.mark.gpu

ARRAYS = ("centers", "ranges", "weights", "left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation")
DARRAYS = ("means", "bandwidth", "bandwidthMin", "bandwidthMax")


def _items():
    """(name, host densities, manifold, mask, Np, Niter)"""
    items = [
        ("euclid 2-D, M = 3", cut_trees(1, 2, [60, 50, 70], [0, 0])[0], None, None, 45, 3),
        ("[e, c], M = 2", cut_trees(2, 2, [50, 60], [0, 1])[0], [0, 1], None, 37, 2),
        ("[e, c], M = 3", cut_trees(3, 2, [50, 60, 40], [0, 1])[0], [0, 1], None, 100, 3),
        ("[c, c], M = 5", cut_trees(4, 2, [30, 40, 50, 35, 45], [1, 1])[0], [1, 1], None, 29, 2),
        ("eec, M = 2", cut_trees(5, 3, [80, 70], [0, 0, 1])[0], [0, 0, 1], None, 51, 2),
        ("[c, c] with a mask", cut_trees(6, 2, [64, 64, 64], [1, 1])[0], [1, 1], [[1, 0], [1, 1], [0, 1]], 43, 2),
        ("refused by the fast forms", refused_trees(7, 2, [24, 31], [0, 1])[0], [0, 1], None, 33, 2),
        # a second 3-D circular item, so that D = 3 is a group (and a batched launch) too; this one records its label trace
        ("cec, M = 3, label trace", cut_trees(8, 3, [60, 75, 50], [1, 0, 1])[0], [1, 0, 1], None, 27, 2),
    ]
    return items


LABELLED = 7            # the item that passes d_labels
# what the mixed batch must launch: the circular fast-mode items of D = 2 (four) and of D = 3 (two) in one launch each; the
# lone Euclidean product and the one the fast forms refuse one by one
WANT_LAUNCHES = {"batched": 2, "singles": 2}


@pytest.fixture(scope="module")
def batch_case():
    """the seven products resident on the device, and the single-call result of each (computed once)"""
    import torch
    dev = torch.device("cuda", 0)
    case = []
    for k, (name, g, man, mask, Np, Niter) in enumerate(_items()):
        dd = [kdehip.DeviceDensity(t) for t in g]
        D, M = dd[0].dims, len(dd)
        P = torch.zeros(D * Np, dtype=torch.float64, device=dev)
        I = torch.zeros(M * Np, dtype=torch.int64, device=dev)
        L = kdehip.nlevels(max(d.num_points for d in dd))
        Lb = torch.zeros(Np * M * L, dtype=torch.int32, device=dev) if k == LABELLED else None
        torch.cuda.synchronize()
        kdehip.prodAppxMSGibbsS_device(dd, P, I, Np=Np, Niter=Niter, seed=900 + k, partialDimMask=mask, manifold=man,
                                       d_labels=Lb)
        torch.cuda.synchronize()
        case.append(dict(name=name, dd=dd, manifold=man, mask=mask, Np=Np, Niter=Niter, seed=900 + k, nlabels=Np * M * L,
                         points=P.cpu().numpy().copy(), indices=I.cpu().numpy().copy(),
                         labels=None if Lb is None else Lb.cpu().numpy().copy()))
    yield case
    for c in case:
        for d in c["dd"]:
            d.close()


def _run_batch(case, order, shared_manifold_arg=False):
    import torch
    dev = torch.device("cuda", 0)
    prods, outs = [], []
    for k in order:
        c = case[k]
        D, M = c["dd"][0].dims, len(c["dd"])
        P = torch.zeros(D * c["Np"], dtype=torch.float64, device=dev)
        I = torch.zeros(M * c["Np"], dtype=torch.int64, device=dev)
        Lb = torch.zeros(c["nlabels"], dtype=torch.int32, device=dev) if c["labels"] is not None else None
        outs.append((P, I, Lb))
        pr = dict(trees=c["dd"], d_points=P, d_indices=I, Np=c["Np"], Niter=c["Niter"], seed=c["seed"],
                  partialDimMask=c["mask"], d_labels=Lb)
        if not shared_manifold_arg:
            pr["manifold"] = c["manifold"]
        prods.append(pr)
    torch.cuda.synchronize()
    if shared_manifold_arg:
        kdehip.prodAppxMSGibbsS_batch(prods, manifold=[case[k]["manifold"] for k in order])
    else:
        kdehip.prodAppxMSGibbsS_batch(prods)
    torch.cuda.synchronize()
    return [(P.cpu().numpy(), I.cpu().numpy(), None if Lb is None else Lb.cpu().numpy()) for P, I, Lb in outs]


def _check(batch_case, order, got):
    for k, (p, i, lab) in zip(order, got):
        c = batch_case[k]
        assert np.array_equal(i, c["indices"]), c["name"]
        assert np.array_equal(p, c["points"]), c["name"]
        if c["labels"] is not None:
            assert lab.any() and np.array_equal(lab, c["labels"]), c["name"]


def test_mixed_batch_equals_the_single_calls(batch_case):
    order = list(range(len(batch_case)))
    for per_call_keyword in (False, True):
        got = _run_batch(batch_case, order, per_call_keyword)
        assert kdehip.batch_launches() == WANT_LAUNCHES   # the circular groups rode the batched instantiation
        _check(batch_case, order, got)
    # the circular items are circular: the same batch without manifolds gives them other numbers
    import torch
    dev = torch.device("cuda", 0)
    c = batch_case[1]
    P = torch.zeros(2 * c["Np"], dtype=torch.float64, device=dev)
    I = torch.zeros(2 * c["Np"], dtype=torch.int64, device=dev)
    kdehip.prodAppxMSGibbsS_batch([dict(trees=c["dd"], d_points=P, d_indices=I, Np=c["Np"], Niter=c["Niter"], seed=c["seed"])])
    torch.cuda.synchronize()
    assert not (np.array_equal(I.cpu().numpy(), c["indices"]) and np.allclose(P.cpu().numpy(), c["points"]))


def test_batch_results_do_not_depend_on_the_order(batch_case):
    order = [3, 7, 6, 1, 0, 5, 2, 4]
    got = _run_batch(batch_case, order)
    assert kdehip.batch_launches() == WANT_LAUNCHES
    _check(batch_case, order, got)


def _same_density(a, b, what=""):
    assert a.bt.dims == b.bt.dims and a.bt.num_points == b.bt.num_points, what
    for name in ARRAYS:
        assert np.array_equal(getattr(a.bt, name), getattr(b.bt, name)), (what, name)
    for name in DARRAYS:
        assert np.array_equal(getattr(a, name), getattr(b, name)), (what, name)


def test_mul_device_batch_rides_the_batched_circular_launch():
    circ = [0, 1]
    sets = []
    for k, M in enumerate((2, 3, 3, 2)):
        g, _ = cut_trees(40 + k, 2, [100] * M, circ)
        sets.append([kdehip.DeviceDensity(t) for t in g])
    seeds = [61, 62, 63, 64]
    try:
        outs = kdehip.mul_device_batch(sets, seeds=seeds, manifold=circ)
        assert kdehip.batch_launches() == {"batched": 1, "singles": 0}   # all four in one launch of the circular mode
        for k, out in enumerate(outs):
            one = kdehip.mul_device(sets[k], seed=seeds[k], manifold=circ)
            _same_density(out.download(), one.download(), f"item {k}")
            assert np.array_equal(out.bw, one.bw) and out.nevals == one.nevals, k
            assert list(out.manifold) == circ
    finally:
        for s in sets:
            for d in s:
                d.close()


_ONE_BY_ONE_SCRIPT = r'''
import numpy as np, torch, kdehip
from tests.circular_plan_cases import cut_trees
dev = torch.device("cuda", 0)
circ, Np, Niter = [0, 1], 37, 2
sets = [[kdehip.DeviceDensity(t) for t in cut_trees(70 + k, 2, [50, 60], circ)[0]] for k in range(3)]
def arrays():
    return ([torch.zeros(2 * Np, dtype=torch.float64, device=dev) for _ in sets],
            [torch.zeros(2 * Np, dtype=torch.int64, device=dev) for _ in sets])
Pb, Ib = arrays()
Ps, Is = arrays()
torch.cuda.synchronize()
kdehip.prodAppxMSGibbsS_batch([dict(trees=s, d_points=Pb[k], d_indices=Ib[k], Np=Np, Niter=Niter, seed=k) for k, s in enumerate(sets)],
                              manifold=circ)
torch.cuda.synchronize()
assert kdehip.batch_launches() == {"batched": 0, "singles": 3}, kdehip.batch_launches()
for k, s in enumerate(sets):
    kdehip.prodAppxMSGibbsS_device(s, Ps[k], Is[k], Np=Np, Niter=Niter, seed=k, manifold=circ)
torch.cuda.synchronize()
assert all(torch.equal(Pb[k], Ps[k]) and torch.equal(Ib[k], Is[k]) for k in range(3))
print("one by one ok")
'''


def test_the_one_by_one_switch_gives_the_same_bytes():
    """KDEHIP_BATCH_CIRC=0 (include/kdehip.h section 2e; read once per process, hence a fresh child): circular items are
    enqueued one by one inside the batch call, as before the batched instantiation existed, with the same results."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, KDEHIP_BATCH_CIRC="0", PYTHONPATH=root)
    out = subprocess.run([sys.executable, "-c", _ONE_BY_ONE_SCRIPT], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "one by one ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
