"""The live frame calls' staging layouts and record structs (csrc/gs_frame_host.hpp), without a GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frame_layouts_under_address_and_undefined_sanitizers(tmp_path):
    """tests/frame_layout_san.cpp: a stand-alone program (its own main, no HIP, nothing loaded into python) around csrc/gs_frame_host.hpp"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "frame_layout_san")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "opendlv-logic-cfsd18-sensation-slam_amd", "csrc"), os.path.join(ROOT, "tests", "frame_layout_san.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "frame layout: ok" in out.stdout, out.stdout + out.stderr
