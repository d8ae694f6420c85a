"""Deterministic mode, CPU side: the switch (`flowhip.set_deterministic`,
`deterministic_enabled`, the `deterministic` context manager, the
FLOWHIP_DETERMINISTIC environment variable), the train CLI's
`--deterministic`, and the PAC predicates stepping aside. The kernels the
mode selects are pinned in tests/test_gpu_deterministic.py."""

import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

import flowhip
from flowhip import ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _restore_mode():
    prev = ops.deterministic_enabled()
    yield
    ops.set_deterministic(prev)


def _child_reports(env_value):
    env = {k: v for k, v in os.environ.items() if k != "FLOWHIP_DETERMINISTIC"}
    if env_value is not None:
        env["FLOWHIP_DETERMINISTIC"] = env_value
    out = subprocess.run(
        [sys.executable, "-c",
         "import sys; sys.path.insert(0, %r); import flowhip; "
         "print(flowhip.deterministic_enabled())" % REPO],
        env=env, check=True, capture_output=True, text=True)
    return out.stdout.strip().splitlines()[-1]


def test_default_is_off():
    assert _child_reports(None) == "False"
    assert _child_reports("0") == "False"


def test_environment_variable_turns_it_on():
    assert _child_reports("1") == "True"


def test_reexported_from_package_root():
    for name in ("set_deterministic", "deterministic_enabled",
                 "deterministic"):
        assert getattr(flowhip, name) is getattr(ops, name)


def test_set_and_query():
    ops.set_deterministic(True)
    assert ops.deterministic_enabled() is True
    ops.set_deterministic(0)
    assert ops.deterministic_enabled() is False


@pytest.mark.parametrize("outer", [False, True])
def test_context_manager_restores(outer):
    ops.set_deterministic(outer)
    with ops.deterministic():
        assert ops.deterministic_enabled() is True
        with ops.deterministic(False):
            assert ops.deterministic_enabled() is False
        assert ops.deterministic_enabled() is True
    assert ops.deterministic_enabled() is outer


@pytest.mark.parametrize("outer", [False, True])
def test_context_manager_restores_when_body_raises(outer):
    ops.set_deterministic(outer)
    with pytest.raises(ZeroDivisionError):
        with ops.deterministic(not outer):
            assert ops.deterministic_enabled() is (not outer)
            1 / 0
    assert ops.deterministic_enabled() is outer


@pytest.mark.parametrize("before", [False, True])
def test_mode_sets_and_restores_torch_conv_flag(monkeypatch, before):
    """The convolutions left on torch (MIOpen backward-weights) repeat only
    under torch.backends.cudnn.deterministic; the mode owns it while on."""
    ops.set_deterministic(False)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", before)
    with ops.deterministic():
        assert torch.backends.cudnn.deterministic is True
        with ops.deterministic(False):
            assert torch.backends.cudnn.deterministic is before
        assert torch.backends.cudnn.deterministic is True
    assert torch.backends.cudnn.deterministic is before


def test_train_parser_flag():
    from flowhip.config.args import build_train_parser
    assert build_train_parser(argv=[]).parse_args([]).deterministic is False
    argv = ["--deterministic"]
    assert build_train_parser(argv=argv).parse_args(argv).deterministic is True


@pytest.mark.parametrize("flag", [False, True])
def test_train_flag_reaches_the_switches(monkeypatch, flag):
    from flowhip.config.args import build_train_parser
    from flowhip.engine import train as train_mod
    argv = ["--deterministic"] if flag else []
    args = build_train_parser(argv=argv).parse_args(argv)

    calls = []
    monkeypatch.setattr(train_mod.ops, "set_deterministic",
                        lambda v: calls.append(("flowhip", v)))
    monkeypatch.setattr(
        torch, "use_deterministic_algorithms",
        lambda mode, **kw: calls.append(("torch", mode, kw)))
    train_mod.apply_deterministic(args)
    if flag:
        assert calls == [("flowhip", True),
                         ("torch", True, {"warn_only": True})]
    else:
        assert calls == []


def test_train_calls_apply_deterministic_first(monkeypatch):
    """train() applies the flag before it builds anything."""
    from flowhip.engine import train as train_mod

    class _Stop(Exception):
        pass

    seen = []

    def _apply(args):
        seen.append(args)
        raise _Stop

    monkeypatch.setattr(train_mod, "apply_deterministic", _apply)
    args = SimpleNamespace(deterministic=True)
    with pytest.raises(_Stop):
        train_mod.train(args)
    assert seen == [args]


def _fake_cuda_fp32(*shape):
    """What the PAC predicates look at in a CUDA fp32 tensor."""
    return SimpleNamespace(is_cuda=True, dtype=torch.float32,
                           shape=torch.Size(shape), dim=lambda: len(shape))


@pytest.fixture
def _fake_ext(monkeypatch):
    from flowhip.ops import functional_pac
    monkeypatch.setattr(functional_pac._ext, "ext", lambda: object())
    monkeypatch.setattr(functional_pac._ext, "force_ref", lambda: False)


def test_pac_predicates_step_aside(_fake_ext):
    from flowhip.ops.functional_pac import (pac_conv_fusable,
                                            pac_kernel_fusable,
                                            pac_pool_fusable)
    guide = _fake_cuda_fp32(2, 8, 16, 20)
    kernel_args = (guide, None, "gaussian", "none", False, (5, 5), (1, 1),
                   (1, 1), (2, 2))
    x = _fake_cuda_fp32(2, 2, 16, 20)
    kernel = _fake_cuda_fp32(2, 1, 5, 5, 16, 20)
    weight = torch.zeros(2, 2, 5, 5)
    conv_args = (x, kernel, weight, 1, 2, 1)
    pool_args = (x, kernel, (5, 5), (1, 1))

    # the arguments describe calls the kernels take ...
    ops.set_deterministic(False)
    assert pac_kernel_fusable(*kernel_args) is True
    assert pac_conv_fusable(*conv_args) is True
    assert pac_pool_fusable(*pool_args) is True
    # ... and deterministic mode sends them to the torch implementation
    with ops.deterministic():
        assert pac_kernel_fusable(*kernel_args) is False
        assert pac_conv_fusable(*conv_args) is False
        assert pac_pool_fusable(*pool_args) is False
    assert pac_kernel_fusable(*kernel_args) is True


def test_alt_corr_backward_message_names_the_mode():
    """The refusal is raised in Python, before any kernel launch."""
    from flowhip.ops.functional import AltCorrLookupFn
    ctx = SimpleNamespace(
        saved_tensors=(torch.zeros(1), torch.zeros(1), torch.zeros(1)),
        needs_input_grad=(False, False, True, True, False, False))
    with ops.deterministic():
        with pytest.raises(RuntimeError, match="deterministic"):
            AltCorrLookupFn.backward(ctx, torch.zeros(1))
