"""CPU: the banded and matrix entry points answer every call that needs no context -- status and
sa_last_error(NULL) text, and which check wins when two would fire -- exactly as tests/golden/banded_errors.json
records (written by tests/golden/make_banded_errors.py; every batch call passes ctx = NULL).  No GPU
compute is called here."""
import collections
import ctypes as C
import importlib.util
import json
import os

import seqalib_amd as sa
from util import GOLDEN

_spec = importlib.util.spec_from_file_location("make_banded_errors", os.path.join(GOLDEN, "make_banded_errors.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

FAMILIES = ["banded", "banded_affine", "banded_matrix", "banded_ends_free", "banded_seeded", "matrix"]


def test_fixture_covers_the_entry_points_and_is_the_generators_case_list():
    recorded = json.load(open(gen.FIXTURE))
    fns = collections.Counter(c["fn"] for c in recorded)
    for fam in FAMILIES:
        assert fns["sa_align_batch_" + fam] > 10 and fns["sa_score_batch_" + fam] > 10, fam
    for q in gen.PLAN_QUERIES:
        assert fns[q] > 10, q
    # the fixture is the generator's case list (inputs), with the recorded answers attached
    assert [{"fn": c["fn"], "args": c["args"]} for c in recorded] == gen.cases()
    assert any(c["rc"] == 0 for c in recorded) and len({c["err"] for c in recorded}) > 40


def test_errors_replay_exactly():
    sa.load_library()
    L = C.CDLL(sa.library_path())   # a handle of its own: run_case types the arguments itself
    recorded = json.load(open(gen.FIXTURE))
    wrong = []
    for k, case in enumerate(recorded):
        got = gen.run_case(L, case)
        if got != (case["rc"], case["err"]):
            wrong.append((k, case["fn"], case["args"], "expected", (case["rc"], case["err"]), "got", got))
    assert not wrong, wrong[:5]
