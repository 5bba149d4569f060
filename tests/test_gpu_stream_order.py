"""Stream order of the enqueue-only entries (include/kdehip.h: "enqueue only on `stream`"), with calls in flight.

Every other GPU test of these entries calls them with the device idle and synchronises before it looks.  Here a stream is held
back by a long sleep kernel while the calls are enqueued behind it, so that the inputs are produced late, the outputs are
consumed and overwritten by later work on the stream without a host wait, and the descriptor and scratch blocks of several
calls (csrc/call_block.hpp, the deferred-release queue of csrc/devmem.cpp) are pending at once.  The rows, their argument sets
and the expected arrays -- the blocking entries' bits -- are in tests/stream_order_cases.py; everything is compared with
np.array_equal, NaNs equal.

Every scenario asserts that the hold was still running when its last enqueue returned (`gate.query()` is False): the hold then
covered every call, and no call waited for its stream -- the header's "does not synchronise the host".  A 50 ms hold is
calibrated once per module from the measured rate of the sleep kernel's clock.  Assertions are made after the streams have been
synchronised, so that a failing test leaves nothing pending.

The blocking entries that take "the hipStream_t that produced" their device matrix and wait for it
(`cases.BLOCKING_WAITS`) have a test of their own at the end: there the hold must be running immediately before the call and
over after it.  Every stream used here is one of the module's two (`_streams()`): a further pool stream would keep a hardware
queue and change which queue the library's preparation stream shares (tests/test_gpu_prodexact.py)."""
import numpy as np
import pytest

import kdehip
from tests import stream_order_cases as cases

pytestmark = pytest.mark.gpu

HOLD_MS = 50.0
ENDED = "hold ended before the calls were enqueued"
_STATE = {}
_ROWS = {}


def _cycles():
    """the sleep count of a HOLD_MS hold: one warm-up sleep, then 10^7 cycles timed between two events"""
    import torch
    if "cycles" not in _STATE:
        torch.cuda._sleep(1_000_000)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(10_000_000)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.0
        per_ms = 10_000_000 / ms
        _STATE["cycles"] = int(HOLD_MS * per_ms)
        print(f"sleep kernel: {per_ms:.0f} cycles per millisecond (10^7 cycles took {ms:.3f} ms); a {HOLD_MS:.0f} ms hold is "
              f"{_STATE['cycles']} cycles")
    return _STATE["cycles"]


def hold(stream):
    """holds `stream` back for HOLD_MS: a sleep kernel and, behind it, the event `gate` that is returned"""
    import torch
    with torch.cuda.stream(stream):
        torch.cuda._sleep(_cycles())
        gate = torch.cuda.Event()
        gate.record(stream)
    return gate


def _streams():
    """(a, b): two side streams, b one whose work runs while a is held (two streams that share a hardware queue would make
    every two-stream scenario fail for a reason outside the library: candidates for b are tried until one runs beside a)"""
    import torch
    if "streams" not in _STATE:
        _cycles()
        a = torch.cuda.Stream()
        b = None
        for attempt in range(8):
            b = torch.cuda.Stream()
            gate = hold(a)
            with torch.cuda.stream(b):
                torch.zeros(8, device="cuda:0").add_(1.0)
            b.synchronize()
            beside = not gate.query()
            a.synchronize()
            if beside:
                break
        print(f"stream b runs beside a held stream a: {beside} (candidate {attempt + 1})")
        _STATE["streams"] = (a, b)
    return _STATE["streams"]


def _fetch(outs, stream):
    """the device arrays on the host, copied on `stream` (and waiting for nothing else)"""
    import torch
    with torch.cuda.stream(stream):
        return {k: v.cpu().numpy() for k, v in outs.items()}


def _clone(outs):
    return {k: v.clone() for k, v in outs.items()}


def _diff(got, want, what):
    """the outputs that are not `want`'s bits, as messages"""
    bad = []
    for k, w in want.items():
        g = np.asarray(got[k]).reshape(w.shape)
        if not np.array_equal(g, w, equal_nan=w.dtype.kind == "f"):
            ne = ~((g == w) | ((g != g) & (w != w))) if w.dtype.kind == "f" else g != w
            bad.append(f"{what}: {k}: {int(ne.sum())} of {w.size} elements differ, first at {int(np.argmax(ne.reshape(-1)))}: "
                       f"got {g.reshape(-1)[int(np.argmax(ne.reshape(-1)))]!r}, want {w.reshape(-1)[int(np.argmax(ne.reshape(-1)))]!r}")
    return bad


def _warm(row, stream):
    """the row's call once, synchronised, with `true`: first-use tables, code objects, the block sizes in the allocation
    cache -- and the synchronised result is the blocking entry's, or nothing below means anything"""
    import torch
    outs = row.new_outputs()
    torch.cuda.synchronize()  # (the fills ran on the default stream, which orders nothing on a side stream)
    row.enqueue(row.args["true"], outs, stream.cuda_stream)
    stream.synchronize()
    bad = _diff(_fetch(outs, stream), row.want["true"], "synchronised warm-up")
    assert not bad, bad


def _row(name):
    if name not in _ROWS:
        try:
            _ROWS[name] = cases.build(name)
        except Exception as e:  # noqa: BLE001  (a row that cannot be built fails every test of it, and is built once)
            _ROWS[name] = e
    if isinstance(_ROWS[name], Exception):
        raise _ROWS[name]
    return _ROWS[name]


def _sequence(row, s, first, second, late_inputs):
    """hold; [inputs <- first]; call into Y; seen1 = clone; [inputs <- second]; call into Y again; seen2 = clone"""
    import torch
    Y = row.new_outputs()
    work = row.work_inputs(second) if late_inputs else None
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        gate = hold(s)
        seen = []
        for setname in (first, second):
            if late_inputs:
                for k, t in work.items():
                    t.copy_(row.args[setname]["inputs"][k], non_blocking=True)
                args = row.with_inputs(setname, work)
            else:
                args = row.args[setname]
            row.enqueue(args, Y, s.cuda_stream)
            seen.append(_clone(Y))
    held = not gate.query()
    s.synchronize()
    assert held, ENDED
    bad = _diff(_fetch(seen[0], s), row.want[first], "seen1") + _diff(_fetch(seen[1], s), row.want[second], "seen2")
    assert not bad, bad


# ---- 1. late inputs, early consumer, inputs overwritten afterwards ---------------------------------------------------------
@pytest.mark.parametrize("name", cases.INPUT_ROWS)
def test_late_inputs_early_consumer_inputs_overwritten(name):
    """the inputs hold `decoy` when the call is made and `true` only once the stream gets there; the consumer of the first
    result and the producer of the second call's inputs follow without a host wait"""
    row, (s, _) = _row(name), _streams()
    _warm(row, s)
    _sequence(row, s, "true", "decoy", late_inputs=True)


# ---- 2. early consumer and reuse of the outputs ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.DENSITY_ROWS)
def test_early_consumer_and_reuse_of_the_outputs(name):
    """two calls into the same outputs, a consumer behind each: the consumer of the first call sees the first call"""
    row, (s, _) = _row(name), _streams()
    _warm(row, s)
    _sequence(row, s, "true", "decoy", late_inputs=False)


# ---- 3. calls in flight on two streams ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.ALL_ROWS)
def test_calls_in_flight_on_two_streams(name):
    """a call pending on the held stream a, three more made and finished on b meanwhile: b never waits for a's work, and the
    blocks of the pending call are not handed to the calls on b"""
    import torch
    row, (a, b) = _row(name), _streams()
    _warm(row, a)
    _warm(row, b)
    Y0 = row.new_outputs()
    Yb = [row.new_outputs() for _ in range(3)]
    torch.cuda.synchronize()
    gate = hold(a)
    row.enqueue(row.args["true"], Y0, a.cuda_stream)
    for k in range(3):
        row.enqueue(row.args[f"alt{k + 1}"], Yb[k], b.cuda_stream)
    b.synchronize()
    held = not gate.query()
    bad = [m for k in range(3) for m in _diff(_fetch(Yb[k], b), row.want[f"alt{k + 1}"], f"alt{k + 1} on b")]
    a.synchronize()
    assert held, ENDED
    bad += _diff(_fetch(Y0, a), row.want["true"], "true on a")
    assert not bad, bad


# ---- 4. calls back to back on one held stream --------------------------------------------------------------------------------
def _back_to_back(row, a, order, check_after):
    import torch
    Y = [row.new_outputs() for _ in order]
    torch.cuda.synchronize()
    gate = hold(a)
    held = None
    for k, setname in enumerate(order):
        row.enqueue(row.args[setname], Y[k], a.cuda_stream)
        if k + 1 == check_after:
            held = not gate.query()
    a.synchronize()
    assert held, ENDED
    bad = [m for k, setname in enumerate(order) for m in _diff(_fetch(Y[k], a), row.want[setname], f"call {k} ({setname})")]
    assert not bad, bad


@pytest.mark.parametrize("name", cases.ALL_ROWS)
def test_six_calls_back_to_back_on_a_held_stream(name):
    """each call needs a descriptor block and a pinned image of its own while the others are pending"""
    row, (a, _) = _row(name), _streams()
    _warm(row, a)
    _back_to_back(row, a, ("true", "alt1", "alt2", "alt3", "decoy", "true"), 6)


def test_nine_products_on_a_held_stream():
    """kdehip_prod_philox_device keeps at most eight calls in flight per device and stream: the ninth may wait for the oldest
    of its own stream, so the hold is looked at after the eighth"""
    row, (a, _) = _row("kdehip_prod_philox_device"), _streams()
    _warm(row, a)
    _back_to_back(row, a, ("true", "alt1", "alt2", "alt3", "decoy", "true", "alt1", "alt2", "alt3"), 8)


# ---- 5. teardown with work in flight ------------------------------------------------------------------------------------------
# (the last row's densities are one resident plan: closing the row is kdehip_product_destroy, which "waits for the device
# first if runs were enqueued")
TEARDOWN_ROWS = ["kdehip_evaluate_device", "kdehip_knn_device_at", "kdehip_sample_device", "kdehip_prod_exact_device",
                 "kdehip_evaluate_varbw_device_at", "kdehip_product_sample_philox"]


def _teardown(name, end):
    import torch
    a, _ = _streams()
    row = cases.build(name)  # densities of its own: they are closed under the call
    try:
        _warm(row, a)
        Y = row.new_outputs()
        torch.cuda.synchronize()
        gate = hold(a)
        row.enqueue(row.args["true"], Y, a.cuda_stream)
        held = not gate.query()
        end(row)  # (may return only after the hold)
        a.synchronize()
        assert held, ENDED
        bad = _diff(_fetch(Y, a), row.want["true"], "after the teardown")
        assert not bad, bad
    finally:
        torch.cuda.synchronize()
        row.close()


@pytest.mark.parametrize("name", TEARDOWN_ROWS)
def test_closing_a_density_under_a_pending_call(name):
    """kdehip_density_free waits for the device first: the call that reads the density still gives its result"""
    _teardown(name, lambda row: row.close())


@pytest.mark.parametrize("name", TEARDOWN_ROWS)
def test_clearing_the_cache_under_a_pending_call(name):
    """kdehip_clear_cache drains the deferred-release queue before it hands the blocks back to the driver"""
    _teardown(name, lambda row: kdehip._clib.kdehip_clear_cache())


# ---- 6. blocking entries that wait for the stream that produces their input ---------------------------------------------------
_BT_ARRAYS = ("centers", "ranges", "weights", "left_child", "right_child", "lowest_leaf", "highest_leaf", "permutation")
_BD_ARRAYS = ("means", "bandwidth", "bandwidthMin", "bandwidthMax")


def _density_arrays(d):
    """every array of a density the library built, and its bandwidth search"""
    host = d.download()
    out = {k: np.asarray(getattr(host.bt, k)) for k in _BT_ARRAYS}
    out.update({k: np.asarray(getattr(host, k)) for k in _BD_ARRAYS})
    out["bw"], out["nevals"] = np.asarray(d.bw), np.asarray([d.nevals])
    return out


@pytest.mark.parametrize("name", cases.BLOCKING_WAITS)
def test_a_blocking_entry_waits_for_the_stream_that_produces_its_matrix(name):
    """kdehip_density_from_device_points[_manifold|_tree]: "`stream` = the hipStream_t that produced it, waited for".  The
    matrix holds a decoy when the call is made; the copy of the true points is pending behind the hold on `a`.  The call
    blocks, so the hold is looked at immediately BEFORE it; the density that comes back is, array for array, the one the
    same entry builds from the true matrix with the device idle."""
    import torch
    a, _ = _streams()
    true, decoy = cases.blocking_case(name)
    d_true, d_decoy = cases._dev(true.T), cases._dev(decoy.T)
    work = d_decoy.clone()
    made = []
    try:
        torch.cuda.synchronize()
        made.append(cases.blocking_build(name, d_true, None))
        made.append(cases.blocking_build(name, d_decoy, None))
        want, other = _density_arrays(made[0]), _density_arrays(made[1])
        # the premise: the decoy's density is another one (its points, its search)
        assert not np.array_equal(want["bw"], other["bw"]) and not np.array_equal(want["means"], other["means"])
        torch.cuda.synchronize()
        gate = hold(a)
        with torch.cuda.stream(a):
            work.copy_(d_true, non_blocking=True)
        held = not gate.query()
        made.append(cases.blocking_build(name, work, a.cuda_stream))
        passed = gate.query()
        a.synchronize()
        assert held, ENDED
        assert passed, "the call returned while the stream it was given was still held"
        bad = _diff(_density_arrays(made[2]), want, "built behind the hold")
        assert not bad, bad
    finally:
        torch.cuda.synchronize()
        for d in made:
            d.close()


def test_nothing_is_left_pending():
    import torch
    torch.cuda.synchronize()
    for row in _ROWS.values():
        if not isinstance(row, Exception):
            row.close()
    _ROWS.clear()
    kdehip._clib.kdehip_clear_cache()
