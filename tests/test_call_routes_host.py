"""``gta_attention``'s routes against the record of the revision before the fused layouts shared one autograd Function
(tests/call_routes_expected.json, written by tests/_call_routes.py on that revision and never regenerated since): for every case of the grid
the same exception with the same message, or the same native entries with the same descriptor flags and optional operands, the same
``table_grads`` keywords, the same kind of return value, the same gradients and the same ``kv_cache`` contents.  No GPU: the native launch
entries are spies.  A case that differs is a change of behaviour."""
import os

import pytest

from tests import _call_routes as R

EXPECTED = R.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "call_routes_expected.json"))
CASES = R.cases()


def test_the_grid_is_the_recorded_one():
    assert sorted(CASES) == sorted(EXPECTED) and len(CASES) > 700


def test_every_native_entry_and_every_kind_of_record_is_there():
    """(the file must not have come out as a list of refusals)"""
    called = {note.split()[0] for rec in EXPECTED.values() for note in rec.get("calls", []) + rec.get("first", [])}
    assert called == set(R.ENTRIES) | {"table_grads"}, sorted(set(R.ENTRIES) - called)
    assert sum("raises" not in rec for rec in EXPECTED.values()) > 100
    assert len({rec["raises"] for rec in EXPECTED.values() if "raises" in rec}) > 45


@pytest.mark.parametrize("name", sorted(CASES))
def test_route(name):
    assert CASES[name]() == EXPECTED[name]
