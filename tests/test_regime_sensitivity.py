"""CPU: the narrow-band inputs of tests/test_gpu_banded_regimes.py can see four faults a banded affine
kernel could have.  Each fault is planted in a copy of tests/banded_affine_model.py (one str.replace whose
old text must occur exactly once, so an edit to the model breaks this test loudly), and the mutant must
give another result than the model on those inputs.  This is a condition on the inputs, checked on the
reference model alone: the GPU tests that compare a kernel with the model on them would fail for a kernel
with the same fault.

The GPU inputs are affine_narrow_pairs() x util.REGIME_AFFINE_BANDED x {LocalGotoh, GlobalGotoh} x
w in (0, 1, 3, 32, 65).  The nine short pairs at w in (0, 1, 3) are searched here: a subset, so a
difference found on it is a difference on the GPU inputs, at a hundredth of the model's time.
"""
import inspect

import pytest

import banded_affine_model as bam
from banded_affine_model import GLOBAL, LOCAL, banded_affine_model
from test_gpu_banded_regimes import AFFINE_NARROW_W, affine_narrow_pairs, narrow_widths
from util import REGIME_AFFINE_BANDED

MUTATIONS = {
    # the X / Y border constant: any large negative value instead of the reference's -10000
    "border": ("BORDER_XY = -10000\n", "BORDER_XY = -10 ** 9\n"),
    # the walk in a vertical gap takes the open term before the extend term when both hold
    "open before extend": ("if typ == 1 and (i - 1, j) in X and X[i, j] == X[i - 1, j] + ge:",
                           "if typ == 1 and X[i, j] != mup and (i - 1, j) in X and X[i, j] == X[i - 1, j] + ge:"),
    # a tie M == X == Y goes to the horizontal gap
    "Y before X": ("if typ == 0 and M[i, j] == X[i, j]:",
                   "if typ == 0 and M[i, j] == X[i, j] and not ((i, j) in Y and M[i, j] == Y[i, j]):"),
    # LocalGotoh ends on the first cell holding the maximum, not the last
    "first maximum": ("h >= best", "h > best"),
}
SHORT = 9
WIDTHS = (0, 1, 3)


def mutant(name):
    old, new = MUTATIONS[name]
    src = inspect.getsource(bam)
    assert src.count(old) == 1, (name, src.count(old))
    scope = {"__name__": "banded_affine_mutant"}
    exec(compile(src.replace(old, new), f"<{name}>", "exec"), scope)
    return scope["banded_affine_model"]


def inputs(args):
    pairs = affine_narrow_pairs()[:SHORT]
    assert max(len(a) + len(b) for a, b in pairs) <= 160 and set(WIDTHS) <= set(AFFINE_NARROW_W)
    return [(algo, a, b, w) for algo in (LOCAL, GLOBAL) for w in narrow_widths(args) if w in WIDTHS for a, b in pairs]


_MODEL = {}


def model(algo, args, a, b, w):
    key = (algo, args, a, b, w)
    if key not in _MODEL:
        _MODEL[key] = banded_affine_model(algo, args, a, b, w)
    return _MODEL[key]


def differs(fn, args):
    """Does the mutant give another result than the model under this scoring (a walk that dead-ends or
    trips one of the model's assertions is another result)?"""
    for algo, a, b, w in inputs(args):
        try:
            if fn(algo, args, a, b, w) != model(algo, args, a, b, w):
                return True
        except AssertionError:
            return True
    return False


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_the_narrow_inputs_see_the_mutant(name):
    fn = mutant(name)
    seen = [args for args in REGIME_AFFINE_BANDED if differs(fn, args)]
    print(f"{name}: differs under {len(seen)} of {len(REGIME_AFFINE_BANDED)} scorings: {seen}")
    assert seen, name
    if name == "border":
        # gap terms in the thousands: the only scorings under which pairs this short show the constant
        assert (-2048, -512, 15, -16, True) in seen and (-6000, -5000, 1, -1, True) in seen, seen
        assert (-3, -1, 15, -16, True) not in seen   # with ordinary gap terms the constant wins no cell here


def test_the_unmutated_copy_is_the_model():
    src = inspect.getsource(bam)
    scope = {"__name__": "banded_affine_copy"}
    exec(compile(src, "<copy>", "exec"), scope)
    args = REGIME_AFFINE_BANDED[5]
    assert not differs(scope["banded_affine_model"], args)
