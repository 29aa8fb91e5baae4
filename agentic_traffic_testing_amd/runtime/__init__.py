"""Native serving runtime (C++ via pybind11): block manager + batch builder, and the
shared-memory step channel used by tensor-parallel ranks.

The extension is built in-tree by ``ops/build.py`` (content-hash stamped); importing this
package (re)builds it when its sources changed, unless ``ATTA_NO_BUILD=1``, in which case
a binary whose embedded ``BUILD_HASH`` does not match the sources is refused.
"""
from __future__ import annotations

import importlib
import os


class StaleNativeBuild(ImportError):
    pass


def _binary_embeds(path, digest: str) -> bool:
    try:
        return digest.encode() in path.read_bytes()
    except OSError:
        return False


def _load():
    from ..ops import build

    # a binary that embeds the current source hash is used as is (checked on the file bytes):
    # no build lock is taken, so a tree built by another user need not be writable
    if os.environ.get("ATTA_NO_BUILD", "0") != "1" and not _binary_embeds(
            build.runtime_so_path(), build.runtime_source_hash()):
        build.build_runtime()  # no-op when the stamp matches the sources
    mod = importlib.import_module("._atta_runtime", __name__)
    want = build.runtime_source_hash()
    if getattr(mod, "BUILD_HASH", None) != want:
        raise StaleNativeBuild(
            f"_atta_runtime was built from other sources (BUILD_HASH "
            f"{getattr(mod, 'BUILD_HASH', None)} != {want}); run "
            "`python -m agentic_traffic_testing_amd.ops.build`")
    return mod


_rt = _load()
BlockManager = _rt.BlockManager
ShmChannel = _rt.ShmChannel
BUILD_HASH = _rt.BUILD_HASH

__all__ = ["BlockManager", "ShmChannel", "BUILD_HASH", "StaleNativeBuild"]
