"""No GPU: the host code of csrc/point_cloud.hip under AddressSanitizer and UndefinedBehaviorSanitizer --
tests/host_san/point_cloud_size_sweep.cpp, a stand-alone program, linked with point_cloud.hip built the same way, sweeps
kbn_point_cloud_workspace_bytes over extreme arguments and the entry point's refusals behind it.  The build helpers are
tests/test_host_sanitizers_cpu.py's (its size_sweep program links a fixed list of sources, which point_cloud.hip is not in).

    python -m pytest tests/test_point_cloud_sanitizers_cpu.py -q
"""
import os

import test_host_sanitizers_cpu as hs
from test_host_sanitizers_cpu import toolchain  # noqa: F401  (the fixture: the build directory, or the module's one skip)


def test_point_cloud_size_sweep(toolchain, capsys):  # noqa: F811
    d = toolchain
    objects = [hs.compile_one(os.path.join(hs.CSRC, "point_cloud.hip"), str(d / "pc_point_cloud.o"), hs.ASAN_UBSAN,
                              ("-ffunction-sections", "-fdata-sections")),
               hs.compile_one(os.path.join(hs.HERE, "point_cloud_size_sweep.cpp"), str(d / "pc_size_sweep.o"), hs.ASAN_UBSAN)]
    exe = hs.link(objects, str(d / "pc_size_sweep"), hs.ASAN_UBSAN, ("-Wl,--gc-sections",))
    status, out = hs.execute([exe])
    with capsys.disabled():
        print("\nhost_san: " + "\n".join(l for l in out.splitlines() if l.startswith(("FAIL", "kbn_"))))
    assert status == 0 and "0 failures" in out, out[-3000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out
    assert "5832 calls" in out      # 18^3: the whole product
