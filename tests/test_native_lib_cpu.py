"""The built kernel library loads on a CPU host (dlopen resolves every symbol: a launcher
declared in kernels.h but left undefined fails here, not on the GPU box) and registers
the ops the Python layer calls."""
import os

import pytest
import torch

from hipserve.ops import library_path


built = pytest.mark.skipif(not os.path.exists(library_path()), reason="hipserve/_C.so not built")


@built
def test_format_tables_agree():
    """The kernels' format table (csrc/include/hipserve/quant_formats.h, through the
    quant_formats op) and hipserve/ops/quant.py FORMATS, row for row: this comparison is
    the only link between the C++ and the Python numbers."""
    from hipserve.ops import load_library, quant as Q

    load_library()
    rows = [ln.split() for ln in torch.ops.hipserve.quant_formats().splitlines()]
    native = [(r[0], *map(int, r[1:4]), *(bool(int(v)) for v in r[4:])) for r in rows]
    assert rows and all(len(r) == 8 for r in rows)
    assert native == [(f.name, f.kqt, f.chunk_bytes, f.sub_shift, f.gguf, f.row_scaled, f.prefill, f.moe)
                      for f in Q.FORMATS]
    assert len(Q.BY_KQT) == len(Q.KERNEL_QT) == len(Q.FORMATS)  # ids and type ids are unique


@built
def test_library_loads_and_registers_ops():
    from hipserve.ops import load_library

    load_library()
    for op in ("decode_gemm_partial", "gguf_gemm_parts", "fp8_untile", "gguf_dequant_tiled", "paged_decode",
               "splitk_add_rmsnorm", "prefill_gemm_packed", "fp8_decode_gemm"):
        assert hasattr(torch.ops.hipserve, op), op
