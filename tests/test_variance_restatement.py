"""CPU-side checks of the VAR / STDDEV aggregates: the restatement the GPU tests compare with (tests/variance_ref.py) against exact
rational arithmetic, the ABI's function ids and the shim's mapping of the reference's names and aliases."""
import os
import random
import re

import pytest

from tests import variance_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", range(6))
def test_restatement_matches_exact_arithmetic(seed):
    rng = random.Random(seed)
    for _ in range(40):
        # (the rounding of a mean of 1e9 is ~1e-7 of a spread of 1: the 1e-6 bound needs a group whose spread is near 1, many values)
        offset, scale = rng.choice([(0.0, 1.0), (0.0, 1e-3), (0.0, 1e6), (1e9, 1.0), (-3e5, 1.0), (-3e5, 1e6)])
        n = rng.randint(30 if offset == 1e9 else 0, 60)
        xs = [None if rng.random() < 0.1 else offset + scale * rng.random() for _ in range(n)]
        # a split into partial states merged in a random order gives the same state as one pass
        cuts = sorted(rng.randint(0, n) for _ in range(3))
        parts = [V.state_of(xs[a:b]) for a, b in zip([0] + cuts, cuts + [n])]
        rng.shuffle(parts)
        merged = (0, 0.0, 0.0)
        for p in parts:
            merged = V.merge(merged, p)
        for func in V.FUNCS:
            exact = V.exact_variance(xs, func)
            for st in (V.state_of(xs), merged):
                got = V.finish(st, func)
                if exact is None:
                    assert got is None
                else:
                    assert got == pytest.approx(exact, rel=1e-6, abs=1e-12), (func, xs)


def test_restatement_known_answers():
    s = V.state_of([1.0, 2.0, 3.0, 4.0])
    assert V.finish(s, "var") == 1.6666666666666667 and V.finish(s, "var_pop") == 1.25
    assert V.finish(s, "stddev") == 1.2909944487358056 and V.finish(s, "stddev_pop") == 1.118033988749895
    one = V.state_of([5.0])
    assert V.finish(one, "var") is None and V.finish(one, "var_pop") == 0.0
    assert all(V.finish(V.state_of([None, None]), f) is None for f in V.FUNCS)


def test_header_declares_the_variance_functions():
    hdr = open(os.path.join(ROOT, "include", "dfgpu.h")).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"DFGPU_AGG_(VAR_SAMP|VAR_POP|STDDEV_SAMP|STDDEV_POP) = (\d+)", hdr)}
    assert got == {"VAR_SAMP": 5, "VAR_POP": 6, "STDDEV_SAMP": 7, "STDDEV_POP": 8}


def test_python_names_and_aliases():
    from datafusion_amd import ops
    want = {"var": 5, "var_samp": 5, "var_sample": 5, "var_pop": 6, "var_population": 6, "stddev": 7, "stddev_samp": 7, "stddev_pop": 8}
    assert {k: ops.AGG_FUNCS[k] for k in want} == want


def test_shim_maps_the_reference_names():
    src = open(os.path.join(ROOT, "shim", "src", "operators.rs")).read()
    arms = {}
    for m in re.finditer(r'((?:"[a-z_]+"\s*\|?\s*)+)=>\s*sys::(DFGPU_AGG_[A-Z_]+)', src):
        for name in re.findall(r'"([a-z_]+)"', m.group(1)):
            arms[name] = m.group(2)
    assert arms["var"] == arms["var_samp"] == arms["var_sample"] == "DFGPU_AGG_VAR_SAMP"
    assert arms["var_pop"] == arms["var_population"] == "DFGPU_AGG_VAR_POP"
    assert arms["stddev"] == arms["stddev_samp"] == "DFGPU_AGG_STDDEV_SAMP"
    assert arms["stddev_pop"] == "DFGPU_AGG_STDDEV_POP"
