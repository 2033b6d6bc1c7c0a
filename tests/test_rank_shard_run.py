"""run.py's KGE_EVAL_SHARDED switch, the part decided before any launch: unset
or 0 is off, and the combinations the sharded evaluation has no form for are
refused with a ValueError."""
from argparse import Namespace

import pytest

from knowledgegraphembedding_amd import run

VARS = ("KGE_EVAL_SHARDED", "KGE_EVAL_CANDIDATES", "KGE_EVAL_RELATIONS")


@pytest.fixture
def env(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def test_off_by_default(env):
    assert run.eval_sharded_requested(Namespace(countries=False)) is False
    for off in ("0", ""):
        env.setenv("KGE_EVAL_SHARDED", off)
        assert run.eval_sharded_requested(Namespace(countries=True)) is False  # nothing is checked when off


def test_on(env):
    env.setenv("KGE_EVAL_SHARDED", "1")
    assert run.eval_sharded_requested(Namespace(countries=False)) is True
    for var in ("KGE_EVAL_CANDIDATES", "KGE_EVAL_RELATIONS"):
        env.setenv(var, "0")  # 0 is "unset" for these too
    assert run.eval_sharded_requested(Namespace(countries=False)) is True


@pytest.mark.parametrize("var,value", [("KGE_EVAL_CANDIDATES", "500"), ("KGE_EVAL_RELATIONS", "1")])
def test_refused_combinations(env, var, value):
    env.setenv("KGE_EVAL_SHARDED", "1")
    env.setenv(var, value)
    with pytest.raises(ValueError, match=var):
        run.eval_sharded_requested(Namespace(countries=False))


def test_refused_with_countries(env):
    env.setenv("KGE_EVAL_SHARDED", "1")
    with pytest.raises(ValueError, match="countries"):
        run.eval_sharded_requested(Namespace(countries=True))
