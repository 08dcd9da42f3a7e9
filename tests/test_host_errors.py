"""Return codes, bj_last_error() strings and the order of the argument checks of the collective, host-commit
and tree ABI, held to tests/golden/host_errors.json, which tools/record_host_errors.py recorded from the
library as it was before these sources took their host helpers from csrc/host.hpp.  The cases are in
tests/host_error_cases.py; none launches anything."""
import json
import os

import pytest

import host_error_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "host_errors.json")))


def _check(which):
    from boojum_amd import _lib
    got = cases.run(_lib.load(), which)
    assert len(got) == len(which), "case names repeat"
    wrong = {n: (g, GOLDEN.get(n)) for n, g in got.items() if g != GOLDEN.get(n)}
    assert not wrong, wrong
    for g in got.values():
        assert g["rc"] in (-22, -5) and g["error"]


def test_golden_covers_exactly_the_cases():
    assert sorted(GOLDEN) == sorted(n for n, _ in cases.HOST + cases.DEVICE)


def test_rejected_calls_without_a_device():
    _check(cases.HOST)


@pytest.mark.gpu
def test_rejected_calls_that_make_a_local_group():
    _check(cases.DEVICE)
