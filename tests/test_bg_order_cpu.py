"""CPU: the two-step background test of the sparse seed pass (csrc/ia3_bgtest.h, compiled with the host compiler): centre
plane first, the outer planes on need, against a literal copy of the sequential 27-value loop: a million random tuples with
many ties (float32 and uint16-quantised), an exhaustive sweep of NaN, +-inf, +-0 and finite values at the centre, an
in-plane and an out-of-plane position, thresholds on either side of diff, cmax = NaN (tests/native/bgtest_cpu.cpp)."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "bgtest_cpu.cpp")
HDR = os.path.join(HERE, "..", "imageanalysis3_amd", "csrc", "ia3_bgtest.h")
EXE = os.path.join(HERE, "native", "bgtest_cpu")


def _build(exe, extra=()):
    if not os.path.isfile(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off"] + list(extra) + ["-o", exe, SRC])
    return exe


def _run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:]
    m = re.search(r"cases (\d+) \(random (\d+), outer planes needed (\d+) of them\), accepted (\d+), outer in all (\d+), mismatches (\d+)",
                  p.stdout)
    assert m, p.stdout
    return [int(v) for v in m.groups()]


def test_two_step_decision_equals_sequential_loop():
    cases, random, outer_random, accepted, outer, bad = _run(_build(EXE))
    assert bad == 0
    assert random == 1000000 and cases > 5 * random
    # every answer of the centre step occurs, among the random tuples too
    assert 0 < outer_random < random and 0 < accepted < cases and 0 < outer < cases


def test_two_step_decision_under_sanitizers():
    """the same stand-alone program with AddressSanitizer and UBSan (a host program of its own: nothing is preloaded)"""
    cases, random, outer_random, accepted, outer, bad = _run(
        _build(EXE + "_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]))
    assert bad == 0 and cases > 5 * random
