"""The owners of device memory, streams and events (smpl_amd/csrc/device_mem.h) compiled for the CPU against a stand-in HIP
runtime (tests/cpp/fake_hip) that keeps the live handles and an ordered log -- with the address and undefined-behaviour
sanitizers, as a program.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owners_free_once_and_in_order(tmp_path):
    """tests/cpp/device_mem_host_driver.cpp: a move leaves exactly one owner and a self-move changes nothing; alloc and create
    on a holder release first; a DevBuf or PinBuf that grows frees the old block once and one that fits does nothing; a
    failed reserve leaves p == nullptr and cap == 0; a struct that declares its stream first destroys it last; in the end
    nothing is live and nothing was released twice"""
    exe = str(tmp_path / "device_mem_host_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "tests", "cpp", "fake_hip"),
                           os.path.join(ROOT, "tests", "cpp", "device_mem_host_driver.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
