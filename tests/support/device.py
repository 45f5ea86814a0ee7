"""The device side of the suite: the package accessor, the module's device fixture, host/device moves of result dicts, a free
rendezvous port and the no-host-read guard."""
import socket

import pytest
import torch


def vml():
    import models
    return models.vml_amd


def _device(load):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def dev():
    """cuda:0 with the HIP library loaded.  A test module imports it by name: pytest registers an imported fixture in the importing
    module, so each module has its own, module-scoped."""
    return _device(vml()._lib.load)


@pytest.fixture(scope="module", name="dev")
def dev_torch():
    """the same under the name dev, with the operator library loaded (load_torch) in place of the C ABI alone"""
    return _device(vml()._lib.load_torch)


def free_port():
    # tests/conftest.py keeps a copy of its own (_free_port): the yardstick files import nothing from here
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def checked_no_sync(fn):
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        return fn()
    finally:
        torch.cuda.set_sync_debug_mode(mode)


def to_dev(r, dev):
    return {key: v.to(dev) for key, v in r.items()}


def to_cpu(r):
    return {key: v.cpu() for key, v in r.items()}


@pytest.fixture()
def gemm_mode():
    """set_gemm_mode, restoring the library's starting mode (_lib.DEFAULT_GEMM_MODE) afterwards"""
    import models
    yield models.vml_amd.set_gemm_mode
    models.vml_amd.set_gemm_mode(models.vml_amd._lib.DEFAULT_GEMM_MODE)
