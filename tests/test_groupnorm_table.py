"""CPU side of tests/test_gpu_groupnorm.py: its table of entry points against include/mulan_hip.h -- every exported
mulan_groupnorm_* function must be named there with the float64-referenced test that calls it."""
import inspect
import os
import re

from tests import test_gpu_groupnorm as gn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exported_groupnorm_entry_points():
    with open(os.path.join(ROOT, "include", "mulan_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)                  # declarations only, not the prose
    return set(re.findall(r"^int\s+(mulan_groupnorm_\w+)\s*\(", text, re.M))


def test_every_groupnorm_entry_point_has_a_float64_test():
    found = exported_groupnorm_entry_points()
    assert {"mulan_groupnorm_fwd", "mulan_groupnorm_bwd_stream", "mulan_groupnorm_stats"} <= found
    assert found == set(gn.COVERAGE), (sorted(found - set(gn.COVERAGE)), sorted(set(gn.COVERAGE) - found))
    source = inspect.getsource(gn)
    for entry, test in gn.COVERAGE.items():
        fn = getattr(gn, test, None)
        assert callable(fn) and test.startswith("test_"), (entry, test)
        assert '"%s"' % entry in source, entry                                  # the name is launched, not only listed
        # the named test reaches the launch helpers that hold that name
        helper = "forward_entry_points" if "_fwd" in entry or entry.endswith("_stats") else "backward_entry_points"
        assert helper in inspect.getsource(fn), (entry, test, helper)
        assert source.count('"%s"' % entry) >= 2, entry                         # the table entry and at least one launch
