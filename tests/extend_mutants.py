"""Faults an extension kernel could have, planted in a copy of tests/extend_model.py: one str.replace on the
module's source whose old text must occur exactly once, so an edit to the model breaks the users of this
file loudly.  tests/test_extend_sensitivity.py shows that the inputs of
tests/test_gpu_banded_extend_regimes.py tell every mutant from the model; the GPU module uses the
"checkpoint at tend" mutant to assert what its phase pairs are for."""
import inspect

import extend_model as em

_BORDER = "                    X[i, j] = Y[i, j] = BORDER_XY\n                continue\n"
MUTATIONS = {
    # the window maximum also takes border cells (the kernel: wmax over `inb` cells, not `interior` ones)
    "recent takes border cells": (_BORDER, _BORDER.replace(
        "                continue\n",
        "                recent = M[i, j] if recent is None else max(recent, M[i, j])\n                continue\n")),
    # border cells other than (0, 0) are end-cell candidates (the kernel: the key is taken from `inb` cells)
    "border cells are candidates": (_BORDER, _BORDER.replace(
        "                continue\n",
        "                if (M[i, j], (i, j)) > (best, end):\n                    best, end = M[i, j], (i, j)\n                continue\n")),
    # the first row-major maximum, not the last
    "first maximum": ("if (v, (i, j)) > (best, end):", "if v > best or (v == best and (i, j) < end):"),
    # best - recent >= xdrop stops
    "stops at equality": ("if xdrop >= 0 and best - recent > xdrop:", "if xdrop >= 0 and best - recent >= xdrop:"),
    # a pair whose last step is a checkpoint step stops there
    "checkpoint at tend": ("if t % XDROP_PERIOD == XDROP_PERIOD - 1 and t < tend:   # a checkpoint",
                           "if t % XDROP_PERIOD == XDROP_PERIOD - 1:   # a checkpoint"),
    # (0, 0) is no candidate: best starts below every score (the kernel: kBandNeg in place of (0, 0)'s key)
    "(0, 0) is no candidate": ("best, end = 0, (0, 0)   # the candidate (0, 0) holds 0", "best, end = -(2 ** 30), (0, 0)"),
    # the window is not reset after a checkpoint that did not stop
    "window not reset": ("            recent = None\n\n    end_i, end_j = end", "            pass\n\n    end_i, end_j = end"),
    # the GlobalGotoh X / Y border constant: any large negative value in place of -10000
    "border constant": ("BORDER_XY = -10000\n", "BORDER_XY = -10 ** 9\n"),
    # the GlobalGotoh walk in a vertical gap takes the open term before the extend term when both hold
    "open before extend": ("if not ((i - 1, j) in X and X[i, j] == X[i - 1, j] + ge):   # the extend term is tried first",
                           "if X[i, j] == M[i - 1, j] + go + ge or not ((i - 1, j) in X and X[i, j] == X[i - 1, j] + ge):"),
}
AFFINE_ONLY = ("border constant", "open before extend")


def mutant(name):
    """extend_model with the named fault (None: an unchanged copy)."""
    src = inspect.getsource(em)
    if name is not None:
        old, new = MUTATIONS[name]
        assert src.count(old) == 1, (name, src.count(old))
        src = src.replace(old, new)
    scope = {"__name__": "extend_mutant"}
    exec(compile(src, f"<{name}>", "exec"), scope)
    return scope["extend_model"]
