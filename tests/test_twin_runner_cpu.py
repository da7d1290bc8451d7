"""tests/_twin.py without a GPU and without the library: the environment run_twin gives its child, what a failing child does to the
test, the bit-for-bit compare.  The children are one-liners that save a part of their own os.environ."""
import pytest
import torch

from _twin import assert_same_dict, run_twin, same_bits

KEYS = ("RDRF_LIB", "RDRF_MARGINS", "RDRF_DETERMINISTIC", "RDRF_FLAT")
ENV_CHILD = ["-c", f"import os, sys, torch; torch.save({{k: os.environ.get(k) for k in {KEYS!r}}}, sys.argv[1])"]


@pytest.fixture
def parent_env(monkeypatch):
    monkeypatch.setenv("RDRF_LIB", "/somewhere/else.so")
    monkeypatch.setenv("RDRF_MARGINS", "/somewhere/margins.txt")
    monkeypatch.setenv("RDRF_DETERMINISTIC", "0")
    monkeypatch.delenv("RDRF_FLAT", raising=False)


def test_child_environment(tmp_path, parent_env):
    env = run_twin(tmp_path, ENV_CHILD, det=True)
    assert env == {"RDRF_LIB": None, "RDRF_MARGINS": None, "RDRF_DETERMINISTIC": "1", "RDRF_FLAT": None}
    assert run_twin(tmp_path, ENV_CHILD, det=False)["RDRF_DETERMINISTIC"] == "0"
    env = run_twin(tmp_path, ENV_CHILD, lib="/a/tools.so", extra_env={"RDRF_FLAT": "1"})
    assert env["RDRF_LIB"] == "/a/tools.so" and env["RDRF_FLAT"] == "1" and env["RDRF_MARGINS"] is None
    assert run_twin(tmp_path, ENV_CHILD, keep_margins=True)["RDRF_MARGINS"] == "/somewhere/margins.txt"
    env = run_twin(tmp_path, ENV_CHILD, det=True, lib="/a/tools.so", extra_env={"RDRF_DETERMINISTIC": "0", "RDRF_LIB": "/b.so"})
    assert env["RDRF_DETERMINISTIC"] == "0" and env["RDRF_LIB"] == "/b.so"      # extra_env wins over the rest


def test_det_none_leaves_the_variable_as_it_found_it(tmp_path, parent_env, monkeypatch):
    assert run_twin(tmp_path, ENV_CHILD)["RDRF_DETERMINISTIC"] == "0"
    monkeypatch.setenv("RDRF_DETERMINISTIC", "1")
    assert run_twin(tmp_path, ENV_CHILD)["RDRF_DETERMINISTIC"] == "1"
    monkeypatch.delenv("RDRF_DETERMINISTIC")
    assert run_twin(tmp_path, ENV_CHILD)["RDRF_DETERMINISTIC"] is None


def test_a_failing_child_fails_the_test_and_is_not_started_again(tmp_path):
    counter = tmp_path / "started.txt"
    code = f"import sys; open({str(counter)!r}, 'a').write('x'); sys.stderr.write('the child says why'); sys.exit(3)"
    with pytest.raises(AssertionError, match="the child says why"):
        run_twin(tmp_path, ["-c", code])
    assert counter.read_text() == "x"


def test_same_bits():
    a = torch.tensor([[1.0, -2.5, 3.0], [0.0, 1e-30, float("inf")]])
    assert same_bits(a, a.clone())
    nan = torch.tensor([0x7FC00001, 0x7FC00000], dtype=torch.int32).view(torch.float32)
    assert bool(torch.isnan(nan).all()) and same_bits(nan, nan.clone()) and not same_bits(nan, nan.flip(0))
    assert not same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not same_bits(a, a.view(torch.int32))                       # the same bytes in another dtype
    assert not same_bits(a, a.reshape(3, 2))
    t = a.t()
    assert not t.is_contiguous() and same_bits(t, t.contiguous())
    for dtype in (torch.bool, torch.uint8, torch.int64, torch.float64, torch.float16):
        x = torch.tensor([0, 1, 1, 1]).to(dtype)
        assert same_bits(x, x.clone()) and not same_bits(x, x.flip(0)), dtype
    assert not same_bits(torch.tensor([0.0], dtype=torch.float64), torch.tensor([-0.0], dtype=torch.float64))
    assert same_bits(torch.empty(0, 3), torch.empty(0, 3)) and not same_bits(torch.empty(0, 3), torch.empty(0, 3, dtype=torch.int32))


def test_assert_same_dict():
    ours = {"a": torch.arange(3.0), "b": torch.ones(2, dtype=torch.int64)}
    assert_same_dict({k: v.clone() for k, v in ours.items()}, ours)
    with pytest.raises(AssertionError, match="keys differ"):
        assert_same_dict({"a": ours["a"]}, ours)
    with pytest.raises(AssertionError, match="b"):
        assert_same_dict({"a": ours["a"], "b": torch.zeros(2, dtype=torch.int64)}, ours)
