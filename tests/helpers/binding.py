"""What the tests of the Python binding's checks share: a stand-in for the library that records the calls that reach it, CPU
tensors that pass for device ones, and a context that never saw a device."""
import types

import pytest
import torch

# host helpers that take no context and touch no device: the recorder may forward them to the real library
HOST_HELPERS = {"p252_merkle4_levels_len", "p252_merkle2_levels_len", "p252_merkle4_depth", "p252_merkle2_depth", "p252_tag",
                "p252_encryption_tag"}


class Recorder:
    """stands in for the library: records every other call and returns P252_OK without forwarding it"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name in HOST_HELPERS:
            return getattr(self.real, name)

        def call(*args):
            self.calls.append(name)
            return 0
        return call


class OnDevice(torch.Tensor):
    """a CPU tensor that reports itself to be on cuda:0 — passes the binding's checks; only the recorder ever sees its address"""

    @property
    def is_cuda(self):
        return True

    def get_device(self):
        return 0


def dev(dtype=torch.int64, n=64):
    return torch.zeros(n, dtype=dtype).as_subclass(OnDevice)  # 512 bytes as int64: more than most calls touch, a forest's levels apart


def _dev(n, dtype=torch.int64):  # (the same tensor for the tests that size every buffer themselves)
    return dev(dtype, n)


def _no_device_context():
    from poseidon252_amd import Context
    ctx = Context.__new__(Context)  # no device: nothing below may reach one
    ctx._h, ctx.device = None, 0
    return ctx


def with_cpu_tensor(args):
    """every variant of `args` with one device tensor (an argument, or an entry of a list / tuple argument) replaced by a CPU one"""
    def cpu(t):
        return torch.zeros_like(t.as_subclass(torch.Tensor))
    for name, v in args.items():
        if isinstance(v, OnDevice):
            yield name, dict(args, **{name: cpu(v)})
        elif isinstance(v, (list, tuple)):
            for i in range(len(v)):
                seq = list(v)
                seq[i] = cpu(seq[i])
                yield "%s[%d]" % (name, i), dict(args, **{name: type(v)(seq)})


@pytest.fixture
def recorder(monkeypatch):
    from poseidon252_amd import _lib
    rec = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", rec)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    return rec
