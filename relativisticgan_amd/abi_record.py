"""Recorder of the C-ABI call stream: every rgan_* call the host makes, in order, with its
scalar arguments, the RganConv / RganPost descriptors decoded and pointers as ``p`` / ``0``.

    with Recorder() as rec:
        ...                      # any host code over kernels.py
    rec.rows                     # ["rgan_conv_fwd(conv[B4 16x8x8->32x4x4 k4 s2 p1 T0], p, ...)", ...]

Diagnostic only: tools/abi_trace.py prints an iteration's rows, tests/test_layer_calls_gpu.py
pins the rows of one fused layer.  The size queries of ``SKIP`` answer a number and launch
nothing; they are left out.
"""
import ctypes

from . import _lib as L

SKIP = {"rgan_conv_workspace", "rgan_bn_partial_bytes", "rgan_bn_dd_partial_bytes", "rgan_conv_bn_segments",
        "rgan_conv_post_segments", "rgan_spectral_batch_ws_bytes", "rgan_spectral_ws_bytes", "rgan_profile_kernel"}


def fmt(a):
    if isinstance(a, (int, float)):
        return repr(a)
    if isinstance(a, ctypes.c_void_p) or a is None:
        return "p" if a is not None and a.value else "0"
    try:
        obj = a._obj  # byref(...)
    except AttributeError:
        return type(a).__name__
    if isinstance(obj, L.RganConv):
        return (f"conv[B{obj.batch} {obj.cin}x{obj.hin}x{obj.win}->{obj.cout}x{obj.hout}x{obj.wout} "
                f"k{obj.kh} s{obj.stride} p{obj.pad} T{obj.transposed}]")
    if isinstance(obj, L.RganPost):
        return f"post[mode{obj.mode} nseg{obj.nseg} S{obj.part_segments}]"
    return type(obj).__name__


class _Proxy:
    def __init__(self, lib, rec):
        self._lib, self._rec = lib, rec

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("rgan_") or name in SKIP:
            return fn
        rec = self._rec

        def wrapped(*args):
            rec.rows.append(f"{name}({', '.join(fmt(a) for a in args)})" + (rec.suffix() if rec.suffix else ""))
            return fn(*args)
        return wrapped


class Recorder:
    """Context manager: while it is open, the library handle of _lib is a proxy that appends
    one row per rgan_* call to ``rows``.  ``suffix``: a callable whose string is appended to
    each row as it is made (abi_trace's Python caller chain)."""

    def __init__(self, suffix=None):
        self.rows, self.suffix = [], suffix

    def __enter__(self):
        self._prev = L.lib()
        L._LIB = _Proxy(self._prev, self)
        return self

    def __exit__(self, *exc):
        L._LIB = self._prev
