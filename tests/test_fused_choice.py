"""CPU test of the k_fused choice (3dscan_amd/csrc/sl3d_fused_choice.h -- the header the library compiles, free of HIP): the rule swept
over the whole run-time domain of a launch against the families the sl3d_fused_*.hip units instantiate (tests/native/fused_choice_check.cpp).
Every key the rule returns is compiled, every compiled key is reached, and there are 530 of them -- exactly the k_fused symbols of the
built library.  The check has teeth: with the families enumerated over a narrower domain it reports keys that are not compiled."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "fused_choice_check.cpp")


def _build(tmp_path, name, *flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *flags, SRC, "-o", exe])
    return exe


def test_every_reachable_key_is_compiled_and_every_compiled_key_reached(tmp_path, scanner_mod):
    exe = _build(tmp_path, "fused_choice_check")
    p = subprocess.run([exe, "names"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.splitlines()[-1].startswith("530 compiled keys, 530 reached"), p.stdout.splitlines()[-1]
    names = set(p.stdout.splitlines()[:-1])
    # ... and they are the instantiations the library holds (each kernel once: its host-side handle, not the launch stub)
    nm = subprocess.run(["nm", "-C", scanner_mod.LIB_PATH], capture_output=True, text=True, check=True).stdout
    built = {line.split(" ", 2)[2].split("(")[0].removeprefix("void ") for line in nm.splitlines() if " sl3d::k_fused<" in line}
    assert built == names, (sorted(built - names)[:5], sorted(names - built)[:5])


@pytest.mark.parametrize("mutant", ["DROP_LARGE_LAUNCHES", "DROP_PLANE_TESTS"])
def test_the_check_objects_to_a_narrower_enumeration(tmp_path, mutant):
    exe = _build(tmp_path, "fused_choice_" + mutant.lower(), "-D" + mutant)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode != 0 and "not compiled: " in p.stdout and " 0 violations" not in p.stdout, p.stdout[-2000:]
