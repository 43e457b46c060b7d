"""CPU: the table of tests/forms_cases.py against the key table the library enumerates (csrc/tune_keys.def through
mxlo_tune_key, which needs no device). A key the library gains fails here until it has a row in FORMS or a reason in
EXCLUDED; a value outside the key's range, a `bitwise` claim without a reason and a code location that exists, an empty shape
list, or exact-reduction inputs whose sums leave the integers Float64 holds exactly fail here too. No device call anywhere in
this file."""
import os
import re

import numpy as np
import pytest

import forms_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table(lo):
    return {k: (d, lo_, hi) for k, d, lo_, hi in lo._lib.tune_keys()}


def test_every_key_has_a_row_or_a_reason(table):
    missing = sorted(set(table) - set(fc.FORMS) - set(fc.EXCLUDED))
    assert not missing, f"tune keys without a row in forms_cases.FORMS or a reason in forms_cases.EXCLUDED: {missing}"
    unknown = sorted((set(fc.FORMS) | set(fc.EXCLUDED)) - set(table))
    assert not unknown, f"forms_cases names keys the library does not enumerate: {unknown}"
    both = sorted(set(fc.FORMS) & set(fc.EXCLUDED))
    assert not both, f"keys both in FORMS and in EXCLUDED: {both}"


def test_exclusions_carry_a_checkable_reason():
    for key, why in list(fc.EXCLUDED.items()) + list(fc.EXCLUDED_VALUES.items()):
        assert isinstance(why, str) and len(why) > 40, key
        for path, name in re.findall(r"(tests/\w+\.py)::(\w+)", why):                 # a named test exists
            with open(os.path.join(ROOT, path)) as f:
                assert f"def {name}(" in f.read(), (key, path, name)
    assert set(fc.EXCLUDED) == {"fused_timeout_ms", "fused_debug_drop", "alias_guard", "graph_direct_max"}
    assert set(fc.EXCLUDED_VALUES) == {("kron_fuse", 2), ("push_posted", 2)}


def test_values_lie_in_the_enumerated_range_and_cover_its_ends(table):
    for key, rows in fc.FORMS.items():
        default, lowest, highest = table[key]
        seen = {default}                         # the default-form result of every row is itself a checked run of the family's runner
        for i, r in enumerate(rows):
            assert r["values"], (key, i)
            for v in r["values"]:
                if v == fc.HI_PER_CU:
                    assert key == "red_blocks_per_cu", key                            # the one key whose ceiling depends on the device
                    seen.add(highest)
                    continue
                assert isinstance(v, int) and lowest <= v <= highest, (key, i, v)
                if key in fc.LISTS:
                    assert v in fc.LISTS[key], (key, v)
                assert (key, v) not in fc.EXCLUDED_VALUES, (key, v)
                seen.add(v)
            for k, v in r["fixed"].items():
                assert k in table and k != key and table[k][1] <= v <= table[k][2], (key, i, k, v)
        want = {lowest, highest, default} - {v for k, v in fc.EXCLUDED_VALUES if k == key}
        assert want <= seen, f"{key}: lowest, highest and default must each be run, missing {sorted(want - seen)}"
        if key in fc.LISTS:
            assert set(fc.LISTS[key]) <= seen, key


def test_bitwise_rows_carry_a_reason_and_a_location_that_exists():
    for key, rows in fc.FORMS.items():
        for i, r in enumerate(rows):
            if not r["bitwise"]:
                continue
            assert r["why"] and r["at"], (key, i)
            path, line = r["at"].rsplit(":", 1)
            with open(os.path.join(ROOT, path)) as f:
                lines = f.readlines()
            assert 1 <= int(line) <= len(lines) and lines[int(line) - 1].strip(), (key, i, r["at"])


def test_shapes_families_and_launch_counts_are_well_formed():
    for key, rows in fc.FORMS.items():
        for i, r in enumerate(rows):
            assert len(r["shapes"]) > 0, (key, i)
            assert isinstance(r["family"], str) and r["family"], (key, i)
            if r["engaged"] is not None:
                assert set(r["engaged"]) == set(r["values"]), (key, i)                # a launch count for every value
                assert all(isinstance(n, int) and n >= 1 for c in r["engaged"].values() for n in (c if isinstance(c, tuple) else (c,))), (key, i)
                assert r["probe"] in r["shapes"], (key, i)
    ids = fc.cases()
    assert len(ids) == len(set(ids))


def test_exact_reduction_inputs_stay_inside_the_integers_of_float64():
    assert fc.DOT_BOUND <= 1 << 10 and max(n for _, n in fc.DOTS) <= 1 << 20
    worst = fc.exact_magnitudes()
    assert isinstance(worst, int) and 0 < worst < 1 << 53, worst
    for t, n in fc.DOTS:                                                              # the operands themselves are exact in Float32
        a, b, want = fc.dot_exact(t, n)
        for x in (a if t == "c128" else (a,)) + (b if t == "c128" else (b,)):
            assert x.dtype == np.int64 and np.abs(x).max() <= fc.DOT_BOUND and x[-1] != 0
    for n in sorted({n for _, _, n in fc.DIAGQN}):
        s, y, d, sums = fc.diagqn_exact(n)
        assert np.abs(s).max() <= fc.DQN_S_BOUND and np.abs(y).max() <= 1 << 10 and d.min() >= 1 and sums[2] > 0
        assert np.array_equal(y.astype(np.float32).astype(np.int64), y)               # (and so are s and d)
