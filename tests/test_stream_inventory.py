"""Every entry point of include/wurm_hip.h that takes a `stream` has a case behind the stream gate (tests/stream_cases.py,
run by tests/test_stream_gate_gpu.py), or a stated reason not to.  An entry point added later without one fails here, on
the CPU."""
import os
import re

from tests import stream_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _with_stream():
    """the prototypes of the header (read as tests/test_abi.py reads them) that have a `stream` parameter"""
    text = open(os.path.join(ROOT, 'include', 'wurm_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    protos = re.findall(r'\b(wurm_[a-z_0-9]+)\s*\(([^)]*)\)\s*;', text)
    return {name for name, params in protos if re.search(r'\bvoid\s*\*\s*stream\b', params)}


def test_the_header_has_launching_entry_points():
    names = _with_stream()
    assert 'wurm_single_step' in names and 'wurm_a2c_ff_league_update_gae' in names and 'wurm_version' not in names
    assert len(names) >= 60


def test_every_entry_point_with_a_stream_has_a_case():
    covered = set()
    for case in stream_cases.CASES:
        assert case.covers, f'{case.name}: declares no entry point'
        covered.update(case.covers)
    names = _with_stream()
    assert not covered - names, f'cases name entry points the header does not declare with a stream: {sorted(covered - names)}'
    for name, reason in stream_cases.NOT_COVERED.items():
        assert name in names and name not in covered and len(reason) > 20, name
    missing = names - covered - set(stream_cases.NOT_COVERED)
    assert not missing, f'no stream case for {sorted(missing)}: add one to tests/stream_cases.py'


def test_case_names_are_unique_and_synchronising_calls_carry_their_line():
    names = [case.name for case in stream_cases.CASES]
    assert len(names) == len(set(names))
    for what, where in stream_cases.SYNCHRONISING.items():
        assert ':' in where and len(where) > 30, what
