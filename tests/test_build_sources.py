"""build.py's source lists against the tree (CPU-only)."""
import os

from swapnet_amd import build


def test_build_lists_match_the_tree():
    """Every *.hip under csrc is in HIP_SOURCES (a unit left out is not linked), every *.h is in HEADERS (a header left out does not
    trigger a rebuild: its objects go stale silently), and every listed file exists."""
    def listed(names):
        return {os.path.normpath(os.path.join(build.CSRC, n)) for n in names}

    def present(suffix):
        return {os.path.join(build.CSRC, f) for f in os.listdir(build.CSRC) if f.endswith(suffix)}

    assert present(".hip") <= listed(build.HIP_SOURCES), sorted(present(".hip") - listed(build.HIP_SOURCES))
    assert present(".h") <= listed(build.HEADERS), sorted(present(".h") - listed(build.HEADERS))
    missing = [p for p in sorted(listed(build.HIP_SOURCES + build.CPP_SOURCES + build.HEADERS)) if not os.path.isfile(p)]
    assert not missing, missing
