"""CPU test of the FCM handle's host-side decisions (uammd_amd/csrc/fcm_prep_state.hpp: which preparation a solve takes, which memsets
precede it, what a step's update does): tests/cxx/fcm_prep_state.cpp, a stand-alone program over that header alone, drives the type
against a model of the device side under the address and undefined-behaviour sanitizers."""
import json
import os
import subprocess
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fcm_prep_state") / "fcm_prep_state")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                        os.path.join(HERE, "cxx", "fcm_prep_state.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def _run(program, args, stdin=None):
    t0 = time.time()
    r = subprocess.run([program] + args, input=stdin, capture_output=True, text=True, timeout=600)
    print(r.stdout[-400:].strip(), f"({time.time() - t0:.1f} s)")
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def test_the_header_is_plain_cxx14(tmp_path):
    """No HIP header, no ROCm include path: the header compiles on its own with every warning on."""
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "fcm_prep_state.hpp"\nint main() { uammd_hip::FcmPrepState s; return s.compactCapacity(); }\n')
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "uammd_amd", "csrc"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    src = open(os.path.join(ROOT, "uammd_amd", "csrc", "fcm_prep_state.hpp")).read()
    assert "#include <hip" not in src and "hipStream_t" not in src


def test_golden_trace_replayed_on_the_cpu(program):
    """The call list of tests/golden/fcm_preparation_trace.json (recorded on the GPU before the decisions moved into the header), with both
    reports at 0 as they are at that size: the state type gives the same (preparation, update) pair after every call, and the device model
    finds none of the invariants broken on the way."""
    with open(os.path.join(HERE, "golden", "fcm_preparation_trace.json")) as fh:
        golden = json.load(fh)
    lines = [f"option slot_refresh {golden['setup']['slot_refresh']}"]
    for c in golden["calls"]:
        if c["op"] == "step":
            lines.append(f"step {c['array']} {c['n']} {int(c['kept'])} {int(c['force'])} {c['stream']}")
        elif c["op"] == "solve":
            lines.append(f"solve {c['array']} {c['n']} {int(c['force'])}")
        elif c["op"] == "move":
            lines.append(f"move {c['array']}")
        else:
            lines.append(f"option {c['name']} {c['value']}")
    out = _run(program, ["replay"], "\n".join(lines) + "\n")
    trace = [[int(w) for w in line.split()] for line in out.splitlines()]
    assert len(trace) == len(golden["trace"]) == 40
    for i, (got, want) in enumerate(zip(trace, golden["trace"])):
        assert got == want, (i, got, want)


def test_every_sequence_of_six_calls_under_the_sanitizers(program):
    """Every sequence of up to 6 letters of the 17-letter alphabet (steps that vouch and that do not, with and without forces, plain solves,
    solves in halves, particles moved, another array, N, stream, `slots` and `bin_ahead` toggled, both reports; and beyond the issue's
    fifteen `atomic_spread` toggled and "the next reserve fails"), slot_refresh = 2: invariants I1 to I7 of the program hold after every
    call (I4 from the second solve after both options went off, see the program), and every launch finds buffers that hold it, also after
    a call that failed in a reserve."""
    out = _run(program, ["enumerate", "6"])
    assert f"enumerated {sum(17 ** k for k in range(1, 7))} sequences" in out and "invariants hold" in out


def test_random_sequences_under_the_sanitizers(program):
    """20 000 random sequences of 200 letters, fixed seed, slot_refresh 2 to 4: what depth 6 cannot reach (a refresh after a long run)."""
    out = _run(program, ["random", "20000", "200"])
    assert "20000 sequences of 200 letters, 4000000 calls: invariants hold" in out
