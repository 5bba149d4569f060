"""The table of tests/stream_order_cases.py covers the ABI: every function of include/kdehip.h that takes a `stream` or a
`streams` parameter is in exactly one of three places -- `ALL_ROWS` (a row, run with calls in flight by
tests/test_gpu_stream_order.py), `BLOCKING_WAITS` (a blocking entry that waits for the stream it is given: one test there) or
`NO_ROW` (neither, with the reason).  A new entry with a stream argument fails here until it has a row or a stated reason.
Needs no GPU: the header is parsed as text, the table is imported without building a row."""
import os
import re

from tests import stream_order_cases as cases

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kdehip.h")


def declared(text):
    """{function name: [parameter names]} of every `kdehip_*` function the header text declares; comments are ignored"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for m in re.finditer(r"\b(kdehip_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        names = []
        for par in m.group(2).split(","):
            words = re.findall(r"[A-Za-z_]\w*", par)
            if words and words != ["void"]:
                names.append(words[-1])
        out[m.group(1)] = names
    return out


def stream_taking(text):
    return sorted(name for name, pars in declared(text).items() if "stream" in pars or "streams" in pars)


def places():
    return {"ALL_ROWS": list(cases.ALL_ROWS), "BLOCKING_WAITS": list(cases.BLOCKING_WAITS), "NO_ROW": list(cases.NO_ROW)}


def test_the_parser_reads_declarations_and_ignores_comments():
    text = """
    /* int kdehip_in_a_comment(void *stream); */
    // int kdehip_in_a_line_comment(void *stream);
    typedef struct kdehip_item { double *d_out; void *stream_like; } kdehip_item;
    int kdehip_plain(const kdehip_item *items, double *d_out /* [n] */,
                     void *stream);
    int kdehip_several(kdehip_item *mp, void *const *streams /* one per device */);
    int kdehip_without(const double *d_stream_of_numbers, int device);
    void kdehip_nothing(void);
    """
    d = declared(text)
    assert d == {"kdehip_plain": ["items", "d_out", "stream"], "kdehip_several": ["mp", "streams"],
                 "kdehip_without": ["d_stream_of_numbers", "device"], "kdehip_nothing": []}
    assert stream_taking(text) == ["kdehip_plain", "kdehip_several"]


def test_every_stream_taking_entry_has_a_row_a_test_or_a_reason():
    with open(HEADER) as f:
        want = stream_taking(f.read())
    assert len(want) >= 40 and "kdehip_evaluate_device" in want   # (the parser found the header's declarations) and "kdehip_product_multi_sample_philox" in want
    where = {}
    for place, names in places().items():
        assert len(names) == len(set(names)), f"{place} names an entry twice"
        for n in names:
            where.setdefault(n, []).append(place)
    missing = [n for n in want if n not in where]
    assert not missing, f"no row, no test and no reason for: {missing}"
    twice = {n: p for n, p in where.items() if len(p) > 1}
    assert not twice, f"in more than one place: {twice}"
    unknown = sorted(n for n in where if n not in want)
    assert not unknown, f"not declared in include/kdehip.h with a stream parameter: {unknown}"


def test_the_table_is_consistent():
    assert set(cases.ALL_ROWS) == set(cases._BUILDERS) and len(cases.ALL_ROWS) == len(cases._BUILDERS)
    assert set(cases.DENSITY_ROWS) <= set(cases._BUILDERS) and set(cases.INPUT_ROWS).isdisjoint(cases.DENSITY_ROWS)
    for name, reason in cases.NO_ROW.items():
        assert isinstance(reason, str) and len(reason.split()) >= 4, name
