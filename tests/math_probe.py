"""ctypes loader of the math probe (tests/probe/math_probe.hip -> carl_amd/lib/libcarl_math_probe.so) and one `run` per
argument layout.  A test library: it is built by carl_amd.build.build_probe (again here, lazily, by content hash) and is
not part of the product.  A missing library is an error, never a skip."""
import ctypes as C
import os

import numpy as np

_vp, _i = C.c_void_p, C.c_int
# entry-point layouts: how many input and output arrays, outputs' columns
KINDS = {"sc": (1, 2, 1), "sc2": (2, 4, 1), "unary": (1, 1, 1), "binary": (2, 1, 1), "qaxis": (2, 1, 4), "lookup2": (2, 1, 6)}
_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is None:
        import torch  # noqa: F401  (first: the library binds to the HIP runtime PyTorch loaded, as carl_amd._lib does)

        from carl_amd import build as B

        path = os.environ.get("CARL_MATH_PROBE_LIB_PATH") or B.build_probe()  # (mutation runs load another build)
        if path is None:
            raise RuntimeError(f"{B.PROBE_SRC} is missing: the math probe cannot be built")
        _lib = C.CDLL(path)
    return _lib


def _fn(entry, n_ptr):
    fn = getattr(load(), "probe_" + entry)  # AttributeError: the probe lacks a kernel the case table names -- an error
    fn.restype, fn.argtypes = _i, [_vp] * n_ptr + [_i, _i, _vp]
    return fn


CANARY = {np.dtype(np.float32): np.float32(-7.25e11), np.dtype(np.float64): np.float64(-7.25e111)}


def run(entry, kind, inputs, out_dtype, device, block=256, n=None, tail=0):
    """Launch `probe_<entry>` over the first n elements of `inputs`; returns the outputs as NumPy arrays of n + tail rows:
    the last `tail` rows are canaries the kernel must not have touched."""
    import torch

    n_in, n_out, cols = KINDS[kind]
    assert len(inputs) == n_in
    n = inputs[0].shape[0] if n is None else n
    dev_in = [torch.as_tensor(np.array(a[:n]), device=device) for a in inputs]
    tdt = torch.float32 if np.dtype(out_dtype) == np.float32 else torch.float64
    outs = [torch.full(((n + tail) * cols,), float(CANARY[np.dtype(out_dtype)]), dtype=tdt, device=device) for _ in range(n_out)]
    stream = torch.cuda.current_stream(device).cuda_stream
    err = _fn(entry, n_in + n_out)(*[t.data_ptr() for t in dev_in], *[t.data_ptr() for t in outs], n, block, stream)
    assert err == 0, f"probe_{entry}: hipError {err}"
    torch.cuda.synchronize(device)
    return tuple(t.cpu().numpy().reshape(n + tail, cols) if cols > 1 else t.cpu().numpy() for t in outs)


def staged_table(device, n_blocks, block):
    """every workgroup's LDS copy of the sin / cos table after SinCosTab::stage: [n_blocks, entries, 2]"""
    import torch

    lib = load()
    entries = lib.probe_tab_entries()
    out = torch.full((n_blocks * entries * 2,), -1.0, dtype=torch.float64, device=device)
    lib.probe_tab_stage.restype, lib.probe_tab_stage.argtypes = _i, [_vp, _i, _i, _vp]
    err = lib.probe_tab_stage(out.data_ptr(), n_blocks, block, torch.cuda.current_stream(device).cuda_stream)
    assert err == 0, f"probe_tab_stage: hipError {err}"
    torch.cuda.synchronize(device)
    return out.cpu().numpy().reshape(n_blocks, entries, 2)
