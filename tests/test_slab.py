"""The slab carver (odigos_amd/csrc/slab.hpp) that every device slab of the
OTLP decoder, the GPU encoder and the groupbytrace store is laid out by, and
the cursor the stage workspaces are laid out by: tests/slab_check.cpp, a plain
host program, checks offsets, sizes, staging copies and a failing need() on
fake buffers, and the offsets of the store's control words (GbtWords,
gbt_layout.hpp).  tests/timed_check.cpp, another, drives the timed launch of the
stage hosts (timed_launch.hpp) against a fake event pool."""
import subprocess
from pathlib import Path


def _run_host_check(tmp_path, name):
    src = Path(__file__).with_name(name + ".cpp")
    exe = tmp_path / name
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe), str(src)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout


def test_slab_carver(tmp_path):
    _run_host_check(tmp_path, "slab_check")


def test_timed_launch_hands_its_events_back(tmp_path):
    _run_host_check(tmp_path, "timed_check")
