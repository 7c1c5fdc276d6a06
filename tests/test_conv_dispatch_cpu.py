"""Which kernels a sparse convolution launches, with which arguments, in which order (lidog_amd/me.py:_conv_rows and its
callers), against the traces of the commit before the route choice was gathered into that one function
(tests/golden/conv_dispatch_trace.json.gz, written by `python tests/conv_trace.py` from that commit: see conv_trace.py
for what is replaced, what runs and how arguments are labelled).  Exact equality, launch by launch: the Python layer
only chooses entry points and arguments, so nothing here is a tolerance.  No GPU: no kernel runs."""
import pytest

import conv_trace


@pytest.fixture(scope="module")
def traces():
    return conv_trace.trace_all(), conv_trace.load_golden()


def _first_difference(got, want):
    """None, or one line that says where a case's trace leaves the recorded one"""
    for i, (g, w) in enumerate(zip(got["launches"], want["launches"])):
        if conv_trace.dumps(g) != conv_trace.dumps(w):
            if g[0] != w[0]:
                return f"launch {i}: {g[0]} instead of {w[0]}"
            args = [j for j, (a, b) in enumerate(zip(g, w)) if conv_trace.dumps(a) != conv_trace.dumps(b)]
            j = args[0] if args else min(len(g), len(w))
            return (f"launch {i} ({w[0]}), argument {j - 1}: {g[j] if j < len(g) else '<missing>'!r} instead of "
                    f"{w[j] if j < len(w) else '<none>'!r}\n      got  {g}\n      want {w}")
    if len(got["launches"]) != len(want["launches"]):
        n = min(len(got["launches"]), len(want["launches"]))
        extra = (got["launches"] if len(got["launches"]) > n else want["launches"])[n]
        return f"{len(got['launches'])} launches instead of {len(want['launches'])}: launch {n} is {extra[0]}"
    for key in ("counts", "stopped_at"):
        if got.get(key) != want.get(key):
            return f"{key}: {got.get(key)!r} instead of {want.get(key)!r}"
    return None


def test_the_matrix_is_the_recorded_one(traces):
    got, want = traces
    assert sorted(got) == sorted(want)
    assert len(want) >= 138 and sum(len(c["launches"]) for c in want.values()) >= 680
    # every sync case got as far as the collective, and no further
    assert all(c["stopped_at"] == "comm.transport" for cid, c in want.items() if cid.endswith("/sync"))


def test_every_case_launches_what_it_launched_before(traces):
    got, want = traces
    bad = [(cid, d) for cid, d in ((cid, _first_difference(got[cid], want[cid])) for cid in sorted(want)) if d]
    assert not bad, f"{len(bad)} of {len(want)} cases differ; the first:\n" + \
        "\n".join(f"  {cid}: {d}" for cid, d in bad[:5])


def test_the_difference_message_names_launch_and_argument():
    a = {"launches": [["k", "x", 1, 2.0], ["r", "t"]], "counts": {"fp32": 1}}
    assert _first_difference(a, a) is None
    b = {"launches": [["k", "x", 1, 2], ["r", "t"]], "counts": {"fp32": 1}}
    assert "launch 0 (k), argument 2" in _first_difference(b, a)        # 2 is not 2.0
    assert "q instead of r" in _first_difference({"launches": [a["launches"][0], ["q"]], "counts": a["counts"]}, a)
    assert "1 launches instead of 2" in _first_difference({"launches": a["launches"][:1], "counts": a["counts"]}, a)
    assert "counts" in _first_difference({"launches": a["launches"], "counts": None}, a)
