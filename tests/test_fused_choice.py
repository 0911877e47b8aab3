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


def _plan_and_rule(tmp_path, scanner_mod):
    import instantiation_plan as IP
    exe = _build(tmp_path, "fused_choice_check")

    def rule(shapes):
        p = subprocess.run([exe, "key"], input="".join(" ".join(map(str, s)) + "\n" for s in shapes), capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        return p.stdout.split("\n")[:len(shapes)]

    names = subprocess.run([exe, "names"], capture_output=True, text=True, timeout=600, check=True).stdout.splitlines()[:-1]
    assert sorted(names) == IP.compiled_keys(scanner_mod.LIB_PATH)
    return IP, names, rule


def test_the_instantiation_plan_reaches_every_compiled_key_by_the_rule(tmp_path, scanner_mod):
    """tests/test_gpu_instantiations.py's plan: every launch's shape is mapped by the rule itself to the key planned for it, and the
    planned keys are exactly the compiled ones (530)."""
    IP, names, rule = _plan_and_rule(tmp_path, scanner_mod)
    ctxs = IP.plan(names)
    assert len(names) == 530
    assert IP.plan_violations(ctxs, names, rule) == []


@pytest.mark.parametrize("narrowing", ["drop_one_key", "wrong_phase"])
def test_the_plan_check_objects_to_a_narrower_plan(tmp_path, scanner_mod, narrowing):
    """The check has teeth: a plan without one key, or with one launch moved to the other selection phase, is refused."""
    import dataclasses
    IP, names, rule = _plan_and_rule(tmp_path, scanner_mod)
    ctxs = IP.plan(names)
    c = next(c for c in ctxs if any(ln.phase == "sparse" for ln in c.launches))
    i = next(i for i, ln in enumerate(c.launches) if ln.phase == "sparse")
    if narrowing == "drop_one_key":
        key = c.launches[i].key
        for d in ctxs:
            d.launches = [ln for ln in d.launches if ln.key != key]
    else:
        c.launches[i] = dataclasses.replace(c.launches[i], phase="dense")
    bad = IP.plan_violations(ctxs, names, rule)
    assert len(bad) == 1 and ("not planned: " in bad[0] or " reaches " in bad[0]), bad
