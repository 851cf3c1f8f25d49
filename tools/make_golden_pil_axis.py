"""tests/golden/pil_lanczos_axis.npz: the whole-axis LANCZOS table of vrg_pil_lanczos_table for an axis longer than 2^24, which no C float
holds exactly -- its sizes, SHA-256, bounds and every 4099th weight (the table itself is 403 MB).  Needs the built library, no GPU.

    python tools/make_golden_pil_axis.py
"""
import ctypes as C, hashlib, os, sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

entry.load_package()
from comfyui_vrgamedevgirl_amd import _hip  # noqa: E402

lib = _hip.host_library()
n_in, n_out, stride = (1 << 24) + 1, 1024, 4099
ksize = int(lib.vrg_pil_lanczos_ksize(n_in, n_out))
table = np.zeros(n_out * (2 + ksize), np.int32)
assert lib.vrg_pil_lanczos_table(n_in, n_out, C.c_void_p(table.ctypes.data), C.c_void_p(table[2 * n_out:].ctypes.data)) == 0
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "pil_lanczos_axis.npz"), sizes=np.array([n_in, n_out, ksize], np.int64),
                    stride=np.int64(stride), bounds=table[:2 * n_out].reshape(-1, 2).copy(), weights=table[2 * n_out::stride].copy(),
                    sha256=np.str_(hashlib.sha256(table).hexdigest()))
