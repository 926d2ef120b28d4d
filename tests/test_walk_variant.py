"""Which instantiation of k_traverse_wide a launch runs (nanort_amd/csrc/walk_variant.h: the pick, the occupancy representative,
the list of the instantiations that exist).  Hit records are bit-identical under every variant, so no parity test can see a
wrong pick: tests/cpp/walk_variant_check.cc prints the picks and this compares them with literals written out by hand — every
row of CONFIGS in test_gpu_launch_variants.py, the custom primitives, the one-level depths, the profiling rows — and sweeps the
whole input space for picks that are not listed or that the kernel's static_asserts refuse."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRI, SPH, CYL = 0, 1, 2


@pytest.fixture(scope="module")
def picker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("walk_variant") / "walk_variant_check")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "nanort_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "walk_variant_check.cc"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    assert r.returncode == 0, r.stdout[-3000:]

    def ask(kind, rows):
        text = "".join("%s %s\n" % (kind, " ".join(str(int(x)) for x in row)) for row in rows)
        r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        out = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
        assert len(out) == len(rows)
        return out

    return ask


def name(row):
    """The kernel's printed name of an output row (as test_gpu_launch_variants.py spells it)."""
    f32, stack, stats, kind, plain, clock, width, order = row[:8]
    b = ("false", "true")
    return "%s, %d, %s, %d, %s, %s, %d, %d" % ("float" if f32 else "double", stack, b[stats], kind, b[plain], b[clock], width, order)


def pick(picker, f32=1, kind=TRI, depth=12, wide4=1, big=0, leaf=1, order4=0, plain=1, stats=0, clock=0, prof=0):
    """(defaults: the fp32 triangle context of test_gpu_launch_variants.py under the default trace options)"""
    row = picker("pick", [(f32, kind, depth, wide4, big, leaf, order4, plain, stats, clock, prof)])[0]
    assert row[8] == 1, row
    return name(row)


def test_rows_of_the_gpu_name_test(picker):
    # (a two-level launch is handed kWide4LdsStack = 12 as its depth, a custom one 10, a one-level one the tunable wide_stack)
    assert pick(picker) == "float, 12, false, 0, true, false, 4, 2"                              # f32_default
    assert pick(picker, plain=0) == "float, 12, false, 0, false, false, 4, 2"                   # f32_cull
    assert pick(picker, order4=1) == "float, 12, false, 0, true, false, 4, 3"                   # order4
    assert pick(picker, leaf=0) == "float, 12, false, 0, true, false, 4, 0"                     # no_leaf_compact
    assert pick(picker, leaf=0, order4=1) == "float, 12, false, 0, true, false, 4, 1"           # no_leaf_compact_order4
    assert pick(picker, big=1) == "float, 12, false, 0, true, false, 4, 6"                      # wide4_big_forced
    assert pick(picker, big=1, plain=0) == "float, 12, false, 0, false, false, 4, 6"            # ... with cull_back_face
    assert pick(picker, big=1, leaf=0) == "float, 12, false, 0, true, false, 4, 4"              # ... without leaf_compact
    assert pick(picker, big=1, leaf=0, plain=0) == "float, 12, false, 0, false, false, 4, 4"
    assert pick(picker, depth=10, wide4=0, leaf=0) == "float, 10, false, 0, true, false, 2, 0"  # no_wide4
    assert pick(picker, f32=0, depth=10, wide4=0, leaf=0) == "double, 10, false, 0, true, false, 2, 0"           # f64_default
    assert pick(picker, f32=0, depth=10, wide4=0, leaf=0, plain=0) == "double, 10, false, 0, false, false, 2, 0"  # f64_cull


def test_order_bits_without_plain_options(picker):
    assert pick(picker, order4=1, plain=0) == "float, 12, false, 0, false, false, 4, 3"
    assert pick(picker, leaf=0, order4=1, plain=0) == "float, 12, false, 0, false, false, 4, 1"
    assert pick(picker, leaf=0, plain=0) == "float, 12, false, 0, false, false, 4, 0"
    assert pick(picker, big=1, order4=1) == "float, 12, false, 0, true, false, 4, 6"  # (64-bit offsets: the reference's slot order only)


def test_custom_primitives(picker):
    for kind in (SPH, CYL):
        for plain in (0, 1):  # (the id tests stay whatever the options)
            assert pick(picker, kind=kind, leaf=0, plain=plain) == "float, 12, false, %d, false, false, 4, 0" % kind
            assert pick(picker, kind=kind, depth=10, wide4=0, leaf=0, plain=plain) == "float, 10, false, %d, false, false, 2, 0" % kind
            # fp64 has no two-level records: wide4 is ignored; and the one-level depth is 10 whatever is handed in
            assert pick(picker, f32=0, kind=kind, leaf=0, plain=plain) == "double, 10, false, %d, false, false, 2, 0" % kind
            assert pick(picker, f32=0, kind=kind, depth=16, wide4=0, leaf=0, plain=plain) == "double, 10, false, %d, false, false, 2, 0" % kind


def test_one_level_depths(picker):
    for f32, t in ((1, "float"), (0, "double")):
        for depth, stack in ((8, 8), (12, 12), (16, 16), (11, 16), (32, 16)):
            for plain in (0, 1):  # (PLAIN exists at the default depth only)
                assert pick(picker, f32=f32, depth=depth, wide4=0, leaf=0, plain=plain) == "%s, %d, false, 0, false, false, 2, 0" % (t, stack)
        assert pick(picker, f32=f32, depth=10, wide4=0, leaf=0, plain=1) == "%s, 10, false, 0, true, false, 2, 0" % t
        assert pick(picker, f32=f32, depth=10, wide4=0, leaf=0, plain=0) == "%s, 10, false, 0, false, false, 2, 0" % t


def test_profiling_rows(picker):
    # two levels per step: counting before time stamps, both PLAIN in the reference's order whatever else is asked
    assert pick(picker, stats=1, prof=1) == "float, 12, true, 0, true, false, 4, 0"
    assert pick(picker, stats=1, clock=1, prof=1) == "float, 12, true, 0, true, false, 4, 0"
    assert pick(picker, clock=1, prof=1) == "float, 12, false, 0, true, true, 4, 0"
    assert pick(picker, clock=1, prof=1, big=1, order4=1, plain=0) == "float, 12, false, 0, true, true, 4, 0"
    for f32, t in ((1, "float"), (0, "double")):  # one level per step at the default depth: counting keeps the id tests
        assert pick(picker, f32=f32, depth=10, wide4=0, leaf=0, stats=1, prof=1) == "%s, 10, true, 0, false, false, 2, 0" % t
        assert pick(picker, f32=f32, depth=10, wide4=0, leaf=0, plain=0, clock=1, prof=1) == "%s, 10, false, 0, true, true, 2, 0" % t
        assert pick(picker, f32=f32, depth=8, wide4=0, leaf=0, stats=1, clock=1, prof=1) == "%s, 8, false, 0, false, false, 2, 0" % t
    # the product library has no such instantiation: the requests are ignored
    assert pick(picker, stats=1, clock=1, prof=0) == "float, 12, false, 0, true, false, 4, 2"
    assert pick(picker, depth=10, wide4=0, leaf=0, plain=0, clock=1, prof=0) == "float, 10, false, 0, false, false, 2, 0"
    assert pick(picker, kind=SPH, leaf=0, stats=1, prof=1) == "float, 12, false, 1, false, false, 4, 0"


def test_occupancy_representatives(picker):
    """What sizes the persistent grid is a representative of the launch's family, NOT the variant launched."""
    rows = [(1, TRI, 12, 1), (1, TRI, 10, 0), (1, TRI, 8, 0), (1, TRI, 12, 0), (1, TRI, 16, 0), (1, TRI, 32, 0), (0, TRI, 10, 0), (0, TRI, 16, 0),
            (1, SPH, 12, 1), (1, SPH, 10, 0), (1, CYL, 12, 1), (1, CYL, 10, 0), (0, SPH, 10, 0), (0, CYL, 10, 1)]
    out = picker("occ", rows)
    assert all(r[8] == 1 for r in out)
    assert [name(r) for r in out] == [
        "float, 12, false, 0, true, false, 4, 0", "float, 10, false, 0, true, false, 2, 0", "float, 8, false, 0, false, false, 2, 0",
        "float, 12, false, 0, false, false, 2, 0", "float, 16, false, 0, false, false, 2, 0", "float, 16, false, 0, false, false, 2, 0",
        "double, 10, false, 0, true, false, 2, 0", "double, 16, false, 0, false, false, 2, 0",
        "float, 12, false, 1, false, false, 4, 0", "float, 10, false, 1, false, false, 2, 0", "float, 12, false, 2, false, false, 4, 0",
        "float, 10, false, 2, false, false, 2, 0", "double, 10, false, 1, false, false, 2, 0", "double, 10, false, 2, false, false, 2, 0"]


def test_every_request_picks_a_variant_that_exists(picker):
    flags = list(itertools.product((0, 1), repeat=5))  # wide4, wide4_big, leaf_items, order4, plain_options
    rows = [(f32, kind, depth) + fl + prof_req + (build,)
            for f32 in (1, 0) for kind in (TRI, SPH, CYL) for depth in (8, 10, 12, 16, 11) for fl in flags
            for prof_req in ((0, 0), (1, 0), (0, 1)) for build in (0, 1)]
    assert len(rows) == 2 * 3 * 5 * 32 * 3 * 2
    occ = picker("occ", [r[:4] for r in rows])
    seen = set()
    for req, got, rep in zip(rows, picker("pick", rows), occ):
        f32, stack, stats, kind, plain, clock, width, order, listed = got
        assert listed == 1, (req, got)            # in the list of the build asked about
        assert rep[8] == 1, (req, rep)            # the representative: in the product library's
        assert (f32, kind) == req[:2] and rep[0] == f32 and rep[3] == kind and (rep[2], rep[5]) == (0, 0), (req, got, rep)
        if not f32:
            assert width == 2 and order == 0, (req, got)
        if not req[10]:
            assert not stats and not clock, (req, got)
        # the static_asserts at the head of k_traverse_wide
        assert width in (2, 4), (req, got)
        assert order == 0 or (width == 4 and f32), (req, got)
        assert (order & 2) == 0 or (kind == TRI and not stats), (req, got)
        assert (order & 4) == 0 or ((order & 1) == 0 and kind == TRI and not stats and not clock), (req, got)
        seen.add(got[:8])
    assert len(seen) == 28 + 6  # every listed instantiation is reachable: 28 in both libraries, 6 more in the profiling one
