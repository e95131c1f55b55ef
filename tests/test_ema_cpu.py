"""--rgan_ema_G without a GPU: the flags, their range check, and the C-ABI's argument checks
(answered on the host before any launch, so dummy pointers are never read)."""
import ctypes

import pytest


def test_flags_default_off_and_range(capsys):
    from relativisticgan_amd.config import make_param, parse
    ns = parse([])
    assert ns.rgan_ema_G == 0.0 and ns.rgan_ema_warmup is True
    p = make_param()
    assert p.rgan_ema_G == 0.0 and p.rgan_ema_warmup is True
    on = parse(["--rgan_ema_G", "0.999", "--rgan_ema_warmup", "False"])
    assert on.rgan_ema_G == 0.999 and on.rgan_ema_warmup is False
    assert parse(["--rgan_ema_G", "0"]).rgan_ema_G == 0.0
    for bad in ("1.0", "-0.1", "nan", "2"):
        with pytest.raises(SystemExit):
            parse(["--rgan_ema_G", bad])
        assert "--rgan_ema_G must lie in [0, 1)" in capsys.readouterr().err, bad


def test_library_exports_and_rejects_malformed_ema_calls():
    """Each malformed call returns RGAN_EINVAL (1001) from the host-side check and launches
    nothing; ntensors = 0 succeeds without a launch (no device is touched either way)."""
    from relativisticgan_amd import _lib
    lib = _lib.lib()
    assert "rgan_ema_update" in _lib.EXPORTED and hasattr(lib, "rgan_ema_update")
    arr = ctypes.c_void_p * 2
    ptrs, nulls = arr(0x1000, 0x2000), arr(0x1000, None)
    numel, neg = (ctypes.c_longlong * 2)(4, 7), (ctypes.c_longlong * 2)(4, -1)
    dummy = ctypes.c_void_p(0x3000)

    def call(n=2, avg=ptrs, params=ptrs, numel=numel, hyper=dummy, count=dummy):
        cast = lambda a: None if a is None else ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
        return lib.rgan_ema_update(n, cast(avg), cast(params), cast(numel), hyper, count, None)

    assert lib.rgan_ema_update(0, None, None, None, None, None, None) == 1001
    for name in ("avg", "params", "numel", "hyper", "count"):
        assert call(**{name: None}) == 1001, name
    assert call(avg=nulls) == 1001 and call(params=nulls) == 1001  # a null tensor inside the arrays
    assert call(n=-1) == 1001
    assert call(numel=neg) == 1001
    assert call(n=0) == 0 and call(n=0, avg=None, params=None, numel=None) == 0


def test_generator_ema_rejects_bad_beta():
    import torch
    from relativisticgan_amd.config import make_param
    from relativisticgan_amd.ema import GeneratorEMA
    from relativisticgan_amd.nets import DCGAN_G
    p = make_param(image_size=32, G_h_size=8, z_size=8)
    state = torch.random.get_rng_state()
    G = DCGAN_G(p)
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            GeneratorEMA(G, p, bad)
    torch.random.set_rng_state(state)
