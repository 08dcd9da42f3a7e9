"""Every rejection of the gate-set validator bj_gate_set_check_h -- its code, its bj_last_error() text and
which of two coexisting faults is reported -- held to tests/golden/gate_check_errors.json, which
tools/record_host_errors.py recorded from the library as it was before interpreted and native segments came
to share their placement checks.  The cases are in tests/gate_check_cases.py; the call is host-only."""
import json
import os

import gate_check_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "gate_check_errors.json")))


def test_golden_covers_exactly_the_cases():
    assert sorted(GOLDEN) == sorted(n for n, _ in cases.HOST)


def test_rejected_images():
    from boojum_amd import _lib
    got = cases.run(_lib.load(), cases.HOST)
    assert len(got) == len(cases.HOST), "case names repeat"
    wrong = {n: (g, GOLDEN.get(n)) for n, g in got.items() if g != GOLDEN.get(n)}
    assert not wrong, wrong
    for g in got.values():
        assert g["rc"] == -22 and g["error"].startswith("gate program: ")


def test_every_message_of_the_validator_is_met():
    """The golden holds every distinct text the validator can give: the strings of its source.  A coverage
    guard that depends on the source's call pattern: it finds the messages as the literal arguments of
    bad("...") in gates.hip, so a message built another way would escape it and a bad("...") inside a comment
    would be counted."""
    import re
    src = open(os.path.join(ROOT, "era-boojum_amd", "csrc", "gates.hip")).read()
    texts = {"gate program: " + t for t in re.findall(r'\bbad\("([^"]+)"\)', src)}
    assert texts and texts == {g["error"] for g in GOLDEN.values()}
