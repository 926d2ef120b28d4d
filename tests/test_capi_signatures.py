"""capi.lib() gives every symbol it binds its argtypes, as many as include/nanort_hip.h declares parameters (no compute: CPU box)."""
import os
import re

from nanort_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nanort_hip.h")


def declared_parameter_counts():
    """{symbol: number of parameters} of every NRT_API declaration: top-level commas + 1, `(void)` counting as 0."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)  # (comments hold commas and parentheses of their own)
    counts = {}
    for name, params in re.findall(r"NRT_API\s+[\w\s\*]+?\b(nrt\w+)\s*\(([^;]*)\)\s*;", src):
        depth, commas = 0, 0
        for ch in params:
            if ch in "([":
                depth += 1
            elif ch in ")]":
                depth -= 1
            elif ch == "," and depth == 0:
                commas += 1
        counts[name] = 0 if params.strip() == "void" else commas + 1
    return counts


def bound_here():
    """The symbols whose signatures capi.lib() itself is responsible for."""
    elsewhere = set(getattr(capi, "BOUND_ELSEWHERE", ()))
    return [s for s in capi.SYMBOLS if s not in elsewhere]


def test_the_header_parses_into_every_symbol():
    counts = declared_parameter_counts()
    assert sorted(counts) == sorted(capi.SYMBOLS)
    assert counts["nrtVersion"] == 0 and counts["nrtDeviceCount"] == 0 and counts["nrtCreate"] == 2
    assert counts["nrtGetTreeBounds_f32"] == 3  # (array parameters: `float bmin_out[3]`)
    assert counts["nrtTraverseBatchesSkipDevice_f64"] == 10


def test_every_bound_symbol_has_argtypes_of_the_declared_length():
    L = capi.lib()
    counts = declared_parameter_counts()
    names = bound_here()
    assert len(names) > 90 and "nrtGetTreeBounds_f32" in names and not any(n.startswith("nrtGroup") for n in names)
    bad = []
    for name in names:
        argtypes = getattr(L, name).argtypes
        if argtypes is None:
            bad.append("%s: no argtypes" % name)
        elif len(argtypes) != counts[name]:
            bad.append("%s: %d argtypes, the header declares %d parameters" % (name, len(argtypes), counts[name]))
    assert not bad, bad


def test_symbols_bound_elsewhere_are_the_group_calls():
    """The explicit list beside the table: declared by the header, exported by the library, bound by nanort_amd/dist.py."""
    assert capi.BOUND_ELSEWHERE and all(n.startswith("nrtGroup") for n in capi.BOUND_ELSEWHERE)
    assert sorted(n for n in declared_parameter_counts() if n.startswith("nrtGroup")) == sorted(capi.BOUND_ELSEWHERE)
    table = [symbol for row in capi.SIGNATURES for symbol, _, _ in capi._bound(row)]
    assert len(table) == len(set(table)) and not set(table) & set(capi.BOUND_ELSEWHERE)
