"""Compression by kernel herding (include/kdehip.h section 5t) without a GPU: the four new symbols and the item struct, the
methods on both classes and nothing new in the package's namespace, every refusal the entries make before they touch a device,
the Python front end's refusals, the Julia shim's calls, and the model of tests/compress_model.py pinned on cases whose answer
is known.

The refusals that read a resident handle (per-point bandwidths without var, a mask bit at or above ndims, M above the
handle's N; an item holds ONE density, so no dimension counts can differ within it -- a bw or manifold of another length is
the front end's to refuse) need real handles: they are in tests/test_gpu_compress.py; here the resident entries are refused
for their NULL handles."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kdehip
from kdehip import _lib
from tests import compress_model as cm
from tests import test_equivariance_table as table
from tests import test_julia_shim_syntax as shim

NO_SUCH_DEVICE = 9999  # an ordinal no machine has: each refusal below is the argument's, not the device's
NEW = ["kdehip_compress", "kdehip_compress_device", "kdehip_compress_device_batch", "kdehip_density_compress_device"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib


def _header():
    return open(os.path.join(ROOT, "include", "kdehip.h")).read()


def test_new_symbols_are_exported_bound_and_declared_under_5t():
    lib = C.CDLL(kdehip.LIB_PATH)
    section = _header()
    section = section[section.index("(5t)"):]
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in section, name
    assert "kdehip_compress_item" in section and "KDEHIP_COMPRESS_ONE_BLOCK_MAX" in section


def test_version_stays_600():
    assert kdehip.version() == 600


def test_the_item_struct_has_the_headers_layout():
    """p, var, M, d_idx and the four optional vectors: 8 eight-byte fields, two words, then out, ks, tree_manifold
    (csrc/compress.hip asserts the same size of the C struct); the field order is the header's"""
    assert C.sizeof(_lib.CCompressItem) == 8 * 8 + 8 + 3 * 8
    assert _lib.CCompressItem.flags.offset == 64 and _lib.CCompressItem.circular_mask.offset == 68
    assert _lib.CCompressItem.out.offset == 72 and _lib.CCompressItem.tree_manifold.offset == 88
    body = _header()
    body = body[body.index("typedef struct kdehip_compress_item"):]
    body = re.sub(r"/\*.*?\*/", "", body[:body.index("} kdehip_compress_item;")], flags=re.S)
    names = re.findall(r"\*?\*?\s*\*?(\w+)\s*[;,]", body)
    assert names == [f[0] for f in _lib.CCompressItem._fields_], names


def test_the_limit_and_the_flag_are_the_headers():
    from kdehip import compress
    hdr = _header()
    assert int(re.search(r"#define KDEHIP_COMPRESS_ONE_BLOCK_MAX (\d+)", hdr).group(1)) % 1024 == 0
    assert int(re.search(r"#define KDEHIP_COMPRESS_STEPWISE (\d+)", hdr).group(1)) == compress._STEPWISE


def test_the_surface_is_methods_only():
    with open(table.INIT) as f:
        names = table.exported(f.read())
    for name in ("compress", "herding_order", "compress_batch"):
        assert callable(getattr(kdehip.DeviceDensity, name)), name
        assert name == "compress_batch" or callable(getattr(kdehip.BallTreeDensity, name)), name
        # no new name in the package (`kdehip.compress`, once imported, is the module)
        assert name not in names and not callable(getattr(kdehip, name, None)), name
    with open(os.path.join(table.PACKAGE, "compress.py")) as f:
        text = f.read()
    assert table.exported(text, imports=False) == []   # every function of the module is private
    with open(table.INIT) as f:
        assert "compress" not in table.imported_modules(f.read())
    assert "compress" in table.unexported_modules(open(table.INIT).read())


def _density(D=2, N=20, bw=0.3, seed=3, w=None):
    rng = np.random.default_rng(seed)
    return kdehip.kde(rng.standard_normal((D, N)), [bw], w)


def _call(p, M, var=None, flags=0, man=None, idx=True, device=NO_SUCH_DEVICE):
    out = np.zeros(max(1, min(int(M), 64)), dtype=np.int64)   # (a refused call writes nothing)
    v = None if var is None else np.ascontiguousarray(var, dtype=np.float64)
    cp = None if p is None else C.byref(p._cstruct())
    return L.kdehip_compress(cp, M, _lib.optr(v, _lib.f64p), flags, _lib.ptr(out, _lib.i64p) if idx else None, None, None, None,
                             device, man)


def _words():
    return L.kdehip_last_error().decode()


def test_null_arguments_are_refused():
    p = _density()
    assert _call(None, 3) == _lib.ERR_ARG and _call(p, 3, idx=False) == _lib.ERR_ARG
    h = C.c_void_p()
    d1 = C.c_void_p(8)  # (never dereferenced: the handle is refused first)
    assert L.kdehip_compress_device(None, 3, None, 0, d1, None, None, None, None, None) == _lib.ERR_ARG
    assert L.kdehip_density_compress_device(None, None, 3, None, None, None, None) == _lib.ERR_ARG
    assert L.kdehip_density_compress_device(C.byref(h), None, 3, None, None, None, None) == _lib.ERR_ARG and not h.value
    assert L.kdehip_compress_device_batch(1, None) == _lib.ERR_ARG
    assert L.kdehip_compress_device_batch(-1, None) == _lib.ERR_ARG
    items = (_lib.CCompressItem * 1)()  # a null handle
    assert L.kdehip_compress_device_batch(1, items) == _lib.ERR_ARG


@pytest.mark.parametrize("M", [0, -1, 21, 2 ** 40])
def test_a_count_outside_1_to_n_is_refused(M):
    assert _call(_density(), M) == _lib.ERR_ARG and "1..N" in _words()


def test_more_than_eight_dimensions_are_refused():
    assert _call(_density(D=9, N=12), 3) == _lib.ERR_UNSUPPORTED and "ndims" in _words()


@pytest.mark.parametrize("bad", [0.0, -0.5, np.inf, np.nan])
def test_a_bad_variance_is_refused(bad):
    assert _call(_density(), 3, var=[0.2, bad]) == _lib.ERR_ARG and "variance" in _words()


@pytest.mark.parametrize("flags", [2, 4, 3, -1, 1 << 30])
def test_unknown_flag_bits_are_refused(flags):
    assert _call(_density(), 3, flags=flags) == _lib.ERR_ARG and "flag" in _words()


def test_a_manifold_byte_above_one_is_refused():
    bad = np.array([0, 2], dtype=np.uint8)
    assert _call(_density(), 3, man=_lib.ptr(bad, _lib.u8p)) == _lib.ERR_ARG and "manifold" in _words()


def test_per_point_bandwidths_need_explicit_variances():
    p = _density()
    N, D = p.bt.num_points, p.bt.dims
    p.bandwidth[(N + 3) * D] *= 2.0  # leaf 3 gets a bandwidth of its own
    assert _call(p, 3) == _lib.ERR_UNSUPPORTED and "per-point" in _words()
    rc = _call(p, 3, var=[0.5, 0.5])   # with variances the call gets as far as the device
    assert rc in (_lib.ERR_ARG, _lib.ERR_NO_DEVICE) and "device" in _words().lower()


def test_two_to_the_31_points_are_refused():
    p = _density()
    big = _lib.CDensity.from_buffer_copy(p._cstruct())
    big.npts = 2 ** 31
    out = np.zeros(4, dtype=np.int64)
    one = np.ones(2)
    rc = L.kdehip_compress(C.byref(big), 3, _lib.ptr(one, _lib.f64p), 0, _lib.ptr(out, _lib.i64p), None, None, None, NO_SUCH_DEVICE, None)
    assert rc == _lib.ERR_ARG and "2^31" in _words()


def test_nothing_to_do_is_ok():
    assert L.kdehip_compress_device_batch(0, None) == _lib.KDEHIP_OK


def test_valid_arguments_only_fail_on_the_device():
    """the same calls with valid arguments get as far as the device: the codes above were the arguments'"""
    p = _density()
    circ = np.array([1, 0], dtype=np.uint8)
    for rc in (_call(p, 1), _call(p, 20), _call(p, 3, var=[0.2, 0.4]), _call(p, 3, flags=1),
               _call(p, 3, man=_lib.ptr(circ, _lib.u8p)), _call(_density(D=8, N=12), 3)):
        assert rc in (_lib.ERR_ARG, _lib.ERR_NO_DEVICE)
        assert "device" in _words().lower()


def _fake_device_density(D=2, N=20):
    """a DeviceDensity that never held a handle (the front end must refuse before it would use one)"""
    fake = kdehip.DeviceDensity.__new__(kdehip.DeviceDensity)
    fake._h = None
    fake._host = None
    fake.dims, fake.num_points, fake.device = D, N, 0
    fake.manifold = fake.tree_manifold = None
    return fake


def test_python_front_end_refusals():
    p, fake = _density(), _fake_device_density()
    for d in (p, fake):
        with pytest.raises(ValueError):
            d.compress()                                  # neither M nor mmd_tol
        for kw in (dict(M=0), dict(M=21), dict(M=2.5), dict(M=3, mmd_tol=-1.0), dict(mmd_tol=float("nan")), dict(M=3, bw=0.0),
                   dict(M=3, bw=[0.1, 0.2, 0.3]), dict(M=3, ks=[-1.0, 1.0]), dict(M=3, manifold=[1]), dict(M=3, manifold=[0, 2]),
                   dict(M=3, tree_manifold=[0, 0, 1])):
            with pytest.raises(ValueError):
                d.compress(**kw)
        for kw in (dict(M=0), dict(M=21), dict(M=None), dict(M=3, bw=-1.0), dict(M=3, manifold=[1, 0, 0])):
            with pytest.raises(ValueError):
                d.herding_order(**kw)
    with pytest.raises(TypeError):
        kdehip.DeviceDensity.compress_batch([fake, p], 3)    # host and resident densities mixed
    with pytest.raises(TypeError):
        kdehip.DeviceDensity.compress_batch([p], 3)
    with pytest.raises(ValueError):
        kdehip.DeviceDensity.compress_batch([fake], 21)
    assert kdehip.DeviceDensity.compress_batch([], 3) == []


def test_julia_shim_calls_the_new_entries_as_the_header_declares_them():
    shim.check_blocks(shim.SHIM)
    code = shim.strip_code(open(shim.SHIM).read())
    params = shim.header_params()
    for name, count in (("kdehip_compress", 10), ("kdehip_density_compress_device", 7)):
        m = re.search(r"ccall\(\(:" + name + r",\s*libkdehip\),\s*Cint,\s*\(([^()]*)\)", code)
        assert m, name
        types = [t.strip() for t in m.group(1).split(",") if t.strip()]
        assert len(types) == len(params[name]) == count
        for jt, ct in zip(types, params[name]):
            assert ct in shim.JULIA_TO_C[jt], (name, jt, ct)
    for fn in ("hip_herding_order", "hip_compress"):
        assert re.search(r"\b" + fn + r"\(", code), fn
    body = code[code.index("function hip_herding_order("):]
    assert "manifold_bytes(" in body[:body.index("\nend")]


# ---- the model itself ----------------------------------------------------------------------------------------------------
def test_model_alternates_between_two_far_clusters_of_unequal_mass():
    """two tight clusters 100 apart holding 2/3 and 1/3 of the mass: z is 2/3 on the one and 1/3 on the other up to the
    clusters' width, a pick adds 1 to r on its own cluster alone, and herding's theory says the picks then follow the masses:
    heavy, light, heavy, heavy, light, heavy, ... -- after 3 k picks 2 k are heavy.  The curve falls over the first picks."""
    rng = np.random.default_rng(11)
    pts = np.hstack([1e-3 * rng.standard_normal((2, 12)), 100.0 + 1e-3 * rng.standard_normal((2, 12))])
    w = np.concatenate([np.full(12, 2.0 / 36.0), np.full(12, 1.0 / 36.0)])
    r = cm.herd(pts, w, np.array([0.5, 0.5]), 12)
    heavy = r["idx"] <= 12
    assert heavy[0] and not heavy[1]
    for k in (1, 2, 3, 4):
        assert heavy[:3 * k].sum() == 2 * k, (k, heavy)
    assert np.all(np.diff(r["mmd2"][:3]) < 0.0) and r["mmd2"][2] < 1e-5
    assert abs(r["self_sum"] - (4.0 / 9.0 + 1.0 / 9.0)) < 1e-5
    assert len(set(r["idx"].tolist())) == 12 and np.all(r["margin"] > 0.0)


def test_model_on_duplicates_picks_in_index_order():
    pts = np.tile(np.array([[0.3], [-1.2], [2.0]]), (1, 9))
    r = cm.herd(pts, np.full(9, 1.0 / 9.0), np.array([0.2, 0.3, 0.4]), 9)
    assert r["idx"].tolist() == list(range(1, 10))
    assert np.all(r["margin"][:-1] == 0.0) and r["margin"][-1] == np.inf      # every step is a tie: the index decides
    assert np.array_equal(r["rpick"], np.arange(9.0)) and np.all(r["zpick"] == r["zpick"][0])
    assert abs(r["mmd2"][-1]) <= 1e-15 and np.all(np.abs(r["mmd2"]) <= 1e-15)  # one point, whatever its copies


def test_model_curve_is_the_mmd_of_the_prefix_and_the_run_is_anytime():
    pts, w = cm.two_clusters(3, 90)
    var = np.array([0.3, 0.2, 0.5])
    r = cm.herd(pts, w, var, 20)
    for m in (1, 7, 20):
        direct = cm.mmd2_direct(pts, w, r["idx"][:m] - 1, var)
        assert abs(r["mmd2"][m - 1] - direct) <= 1e-13 * (r["self_sum"] + 2.0 + 1.0)
        short = cm.herd(pts, w, var, m)
        assert np.array_equal(short["idx"], r["idx"][:m]) and np.array_equal(short["rpick"], r["rpick"][:m])
    assert r["idx"][0] == int(np.argmax(r["z"])) + 1
    blocked = cm.herd(pts, w, var, 20, rows=32)                    # three row blocks, the last one partial
    assert np.array_equal(blocked["idx"], r["idx"]) and np.abs(blocked["z"] - r["z"]).max() <= 1e-15


def test_model_wraps_across_the_cut_of_the_circle():
    pts, w = cm.cut_pair()
    var = np.array([0.3, 0.2])
    on, off = cm.herd(pts, w, var, 12, man=[0, 1]), cm.herd(pts, w, var, 12)
    assert np.abs(pts[1][:, None] - pts[1][None, :]).max() > np.pi         # some pairs are 2 pi apart on the line
    assert on["self_sum"] > 1.2 * off["self_sum"]                          # ... and near on the circle
    shifted = pts + np.array([[0.0], [2.0 * np.pi]])
    again = cm.herd(shifted, w, var, 12, man=[0, 1])
    assert np.array_equal(again["idx"], on["idx"]) and abs(again["self_sum"] - on["self_sum"]) <= 1e-12
