"""Write tests/golden/msr_reference.npz from the reference's own vrgdg_ltx_msr_reference_builder.py.  Works only where the reference
checkout exists (VRGDG_REFERENCE_ROOT, see oracle/reference_loader.py).

    python tools/make_golden_msr.py

The module is loaded with a stand-in ``folder_paths`` over a temporary directory of the seeded PNGs of tests/msr_support.py and a stand-in
``cv2`` whose ``resize`` is the numpy restatement of tests/lanczos_support.py (no cv2 is installed where this runs: equality with cv2
itself is pinned by tests/test_gpu_msr.py::test_msr_equals_cv2 wherever cv2 or its fixture exists).  Recorded: the stored bytes of every
input, both classes' surface as JSON, the builder's frames and the loader's five outputs per case -- as bytes: output x 255 is an exact
integer, checked here."""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import msr_support as M                        # noqa: E402
from lanczos_support import restated           # noqa: E402
from oracle import reference_loader as RL      # noqa: E402


def as_bytes(t):
    a = t.numpy()
    b = np.rint(a * np.float32(255.0)).astype(np.uint8)
    assert np.array_equal(M.unit(b), a), "an output is not byte / 255"
    return b


def load_reference():
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LANCZOS4 = 4

    def resize(image, size, interpolation=None):
        assert interpolation == cv2.INTER_LANCZOS4
        return np.ascontiguousarray(restated(np.ascontiguousarray(image)[None], int(size[0]), int(size[1]))[0])

    cv2.resize = resize
    sys.modules["cv2"] = cv2
    path = os.path.join(RL.REFERENCE_ROOT, "vrgdg_ltx_msr_reference_builder.py")
    spec = importlib.util.spec_from_file_location("_vrgdg_reference_msr", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    arrays = {}
    with tempfile.TemporaryDirectory() as directory:
        M.write_inputs(directory)
        before = M.install_folder_paths(directory)
        try:
            ref = load_reference()
            for name in M.PICTURES:
                arrays[f"in.{name}"] = M.picture(name)
            turned = M.decoded(directory, "turned.png")
            assert turned.shape[:2] == (90, 50), "the EXIF orientation was not applied"
            doc = M.surface(ref)
            doc["images"] = [M.NONE_IMAGE] + sorted(M.PICTURES)
            arrays["surface"] = np.array(json.dumps(doc, sort_keys=True))
            for name, case in M.BUILDER_CASES.items():
                (out,) = ref.VRGDG_LTXMSRReferenceBuilder().build_reference(**case)
                arrays[f"builder.{name}"] = as_bytes(out)
            for name, case in M.LOADER_CASES.items():
                outs = ref.VRGDG_LTX25MSRReferenceLoader().load_references(**case)
                arrays[f"loader.{name}.present"] = np.array([o is not None for o in outs])
                for i, o in enumerate(outs):
                    if o is not None:
                        arrays[f"loader.{name}.{i}"] = as_bytes(o)
        finally:
            M.restore_folder_paths(before)
            sys.modules.pop("cv2", None)
    np.savez_compressed(M.FIXTURE, **arrays)
    print(M.FIXTURE, os.path.getsize(M.FIXTURE), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
