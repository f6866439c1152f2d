"""``ops.kernels.rule_combine``: the one table from a rule to the combine of its launch. The
expected plans are written out: they are what ``aggregate`` and the engine's three ladders passed
to ``agg_update`` / ``agg_update_multi`` before the table existed."""
import pytest
import torch

from consensusml_amd.config import RULES
from consensusml_amd.ops import kernels as K

WEIGHTED = dict(combine="weighted", lo=0, cnt=1, keep=None, rows=None, mix=None)
SORTED = dict(combine="sorted", w=None, rows=None)
# rule -> (scalar fields, the tensor fields that are set)
PLANS_7_1 = {     # n = 7, f = 1, trim = None
    "mean": (dict(WEIGHTED, n=7), "w"),
    "median": (dict(SORTED, n=7, lo=3, cnt=1, keep=0), "mix"),
    "trimmed_mean": (dict(SORTED, n=7, lo=1, cnt=5, keep=0), "mix"),
    "meamed": (dict(SORTED, n=7, lo=3, cnt=1, keep=6), "mix"),
    "phocas": (dict(SORTED, n=7, lo=1, cnt=5, keep=6), "mix"),
    "krum": (dict(WEIGHTED, n=7), "w"),
    "multi_krum": (dict(WEIGHTED, n=7), "w"),
    "geomed": (dict(WEIGHTED, n=7), "w"),
    "bulyan": (dict(combine="sorted", n=5, lo=1, cnt=3, keep=None, w=None, mix=None), "rows"),
    "centered_clip": (dict(WEIGHTED, n=8), "w"),        # rows_total = n + 1
}
PLANS_8_2_1 = {   # n = 8, f = 2, trim = 1
    "mean": (dict(WEIGHTED, n=8), "w"),
    "median": (dict(SORTED, n=8, lo=3, cnt=2, keep=0), "mix"),
    "trimmed_mean": (dict(SORTED, n=8, lo=1, cnt=6, keep=0), "mix"),
    "meamed": (dict(SORTED, n=8, lo=3, cnt=2, keep=6), "mix"),
    "phocas": (dict(SORTED, n=8, lo=1, cnt=6, keep=6), "mix"),
    "krum": (dict(WEIGHTED, n=8), "w"),
    "multi_krum": (dict(WEIGHTED, n=8), "w"),
    "geomed": (dict(WEIGHTED, n=8), "w"),
    "bulyan": None,     # the f-trimmed mean of n - 2f = 4 selected rows does not exist at f = 2
    "centered_clip": (dict(WEIGHTED, n=9), "w"),
}


@pytest.mark.parametrize("n,f,trim,plans", [(7, 1, None, PLANS_7_1), (8, 2, 1, PLANS_8_2_1)],
                         ids=["n7-f1", "n8-f2-trim1"])
@pytest.mark.parametrize("rule", RULES)
def test_plan_of_every_rule(rule, n, f, trim, plans):
    assert set(plans) == set(RULES)
    w, sel, M = torch.zeros(n + 1), torch.zeros(n + 1, dtype=torch.int32), torch.eye(n)
    kw = dict(w=w, sel=sel, mix=M, rows_total=n + 1 if rule == "centered_clip" else None)
    if plans[rule] is None:
        with pytest.raises(ValueError, match="trimmed_mean needs n > 2\\*trim"):
            K.rule_combine(rule, n, f, trim, **kw)
        return
    scalars, tensor = plans[rule]
    c = K.rule_combine(rule, n, f, trim, **kw)
    got = c.kwargs()
    assert sorted(got) == ["cnt", "combine", "keep", "lo", "mix", "n", "rows", "w"]
    for key, want in scalars.items():
        assert got[key] == want and type(got[key]) is type(want), (key, got[key], want)
    assert set(scalars) | {tensor} == set(got)
    if tensor == "w":
        assert c.w is w
    elif tensor == "mix":
        assert c.mix is M
    else:       # Bulyan's selection: the first n - 2f entries of the persistent buffer
        assert c.rows.data_ptr() == sel.data_ptr() and tuple(c.rows.shape) == (n - 2 * f,)
    with pytest.raises(AttributeError):     # frozen
        c.n = 0


@pytest.mark.parametrize("rule,n,f,trim,msg", [
    ("meamed", 4, 2, None, "meamed needs n > 2f"),
    ("phocas", 4, 2, 0, "phocas needs n > 2f"),
    ("phocas", 5, 1, 3, "phocas needs n > 2\\*trim"),
    ("trimmed_mean", 4, 0, 2, "trimmed_mean needs n > 2\\*trim"),
    ("trimmed_mean", 4, 2, None, "trimmed_mean needs n > 2\\*trim"),
    ("spectral", 7, 1, None, "unknown rule 'spectral'"),
])
def test_plan_errors(rule, n, f, trim, msg):
    with pytest.raises(ValueError, match=msg):
        K.rule_combine(rule, n, f, trim, w=torch.zeros(n), sel=torch.zeros(n + 1),
                       mix=torch.eye(n))
