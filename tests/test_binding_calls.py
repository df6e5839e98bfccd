"""CPU test of what the Python binding hands to the library: every case of binding_call_cases.py runs against a recording
fake of libo3dr (no built library, no GPU) and must make the calls tests/golden/binding_calls.json holds - the same
symbols, scalars and struct fields, every pointer NULL / an input / an output / something else as it was, and the same
return shapes, dtypes and dataclasses.  The golden file was written from the binding before its intakes, allocator and
result path were unified (python tests/binding_call_cases.py --write against that api.py) and is never regenerated from
the code under test."""
import pytest

import binding_call_cases as B

CASES = B.cases()


@pytest.fixture(scope="module")
def golden():
    return B.load_golden()


@pytest.fixture()
def fake(monkeypatch):
    return B.install(monkeypatch.setattr)


def test_golden_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(c[0] for c in CASES) and len(golden) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_calls_match_golden(case, golden, fake):
    o3dr, lib = fake
    got = B.run_case(o3dr, lib, case)
    want = golden[case[0]]
    assert got == want, f"{case[0]}: " + B.first_difference(want, got)
