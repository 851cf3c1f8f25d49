"""The stream-order probe table (tests/stream_support.py) names every function and method of the package that hands the current stream to
the library.  No GPU is needed."""
import importlib
import inspect
import os
import re

import stream_support as S
from conftest import PKG_DIR


def _takes_the_stream(fn) -> bool:
    return "_hip.current_stream()" in inspect.getsource(inspect.unwrap(fn))


def _stream_takers(module, qualify: bool):
    """names of the module-level functions, and of the methods of its classes, whose source passes _hip.current_stream() on"""
    prefix = module.__name__.rsplit(".", 1)[-1] + "." if qualify else ""
    names = set()
    for name, obj in vars(module).items():
        if getattr(obj, "__module__", None) != module.__name__:
            continue
        if inspect.isfunction(obj):
            if _takes_the_stream(obj):
                names.add(prefix + name)
        elif inspect.isclass(obj) and qualify:            # (ops.HipEvent's methods are the event helpers: no device input)
            for attr, member in vars(obj).items():
                if inspect.isfunction(member) and _takes_the_stream(member):
                    names.add(f"{prefix}{name}.{attr}")
    return names


def test_every_stream_taking_function_is_probed_or_excluded_with_a_reason(pkg):
    takers = set()
    for name in S.STREAM_MODULES:
        module = importlib.import_module(f"comfyui_vrgamedevgirl_amd.{name}")
        found = _stream_takers(module, qualify=name != "ops")
        assert found, name
        takers |= found
    assert len(takers) >= 55, sorted(takers)                      # the scan itself found them (decorated functions are unwrapped)
    covered = S.covered()
    assert covered <= takers, f"stale names in the table: {sorted(covered - takers)}"
    missing = takers - covered - set(S.EXCLUDED)
    assert not missing, f"not in the probe table of tests/stream_support.py: {sorted(missing)}"
    assert set(S.EXCLUDED) <= S.MAY_BE_EXCLUDED and all(isinstance(r, str) and r.strip() for r in S.EXCLUDED.values())
    assert not set(S.EXCLUDED) & covered


def test_no_other_module_hands_the_stream_to_the_library():
    """STREAM_MODULES is the whole list: a new module that calls _hip.current_stream() has to be added to it (and then probed)"""
    found = set()
    for entry in sorted(os.listdir(PKG_DIR)):
        if entry.endswith(".py") and entry != "_hip.py":
            with open(os.path.join(PKG_DIR, entry), encoding="utf-8") as fh:
                if re.search(r"_hip\.current_stream\(\)", fh.read()):
                    found.add(entry[:-3])
    assert found == set(S.STREAM_MODULES), sorted(found ^ set(S.STREAM_MODULES))


def test_the_table_is_consistent():
    names = [c.name for c in S.CASES]
    assert len(names) == len(set(names))
    assert set(S.HOST_SYNCING) <= set(names), sorted(set(S.HOST_SYNCING) - set(names))
    assert all(".py" in where for where in S.HOST_SYNCING.values())
    # a first use uploads its table synchronously: every such case is listed as waiting on the host
    assert all(c.name in S.HOST_SYNCING for c in S.CASES if c.reset is not None)
