"""The slab carver (odigos_amd/csrc/slab.hpp) that every device slab of the
OTLP decoder, the GPU encoder and the groupbytrace store is laid out by:
tests/slab_check.cpp, a plain host program, checks offsets, sizes, staging
copies and a failing need() on fake buffers."""
import subprocess
from pathlib import Path


def test_slab_carver(tmp_path):
    src = Path(__file__).with_name("slab_check.cpp")
    exe = tmp_path / "slab_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), str(src)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout
