"""CPU test of the FCM launch choices (uammd_amd/csrc/fcm_launch_choice.hpp: which instantiation a spread or a gather launches, on how
many workgroups): tests/cxx/fcm_launch_choice.cpp, a stand-alone program over that header alone, under the address and
undefined-behaviour sanitizers."""
import json
import os
import subprocess
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FORMS = {"atomic": 0, "tile": 1, "prep": 2, "inter": 3, "col": 4, "half": 5}   # UAMMD_FCM_GATHER_* of include/uammd_hip.h


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fcm_launch_choice") / "fcm_launch_choice")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                        os.path.join(HERE, "cxx", "fcm_launch_choice.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def _run(program, args, stdin=None):
    t0 = time.time()
    r = subprocess.run([program] + args, input=stdin, capture_output=True, text=True, timeout=600)
    print(r.stdout[-400:].strip(), f"({time.time() - t0:.1f} s)")
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_the_header_is_plain_cxx14(tmp_path):
    """No HIP header, no ROCm include path, no environment: the header compiles on its own with every warning on."""
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "fcm_launch_choice.hpp"\nint main() { return uammd_hip::fcm_choose_gather(uammd_hip::FcmGatherInputs{}).form; }\n')
    r = subprocess.run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "uammd_amd", "csrc"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in ("fcm_launch_choice.hpp", "fcm_prep_state.hpp"):
        src = open(os.path.join(ROOT, "uammd_amd", "csrc", name)).read()
        assert "#include <hip" not in src and "hipStream_t" not in src and "getenv" not in src, name


def _gather_line(cells, support, options, packed, ran):
    if ran == "refused":
        said = [-1, 0, 0, 0, 0]
    else:
        form, rs, p, szmax = ran.split("/")
        said = [FORMS[form], rs, p, szmax, int(form == "inter" and packed)]   # (info's packed flag: the interleaved form read a packed grid)
    return " ".join(map(str, ["gather", *cells, *support, options.get("atomic_spread", 0), options.get("interleaved_gather", 1),
                              options.get("tile_gather", 0), options.get("gather_per_wave", 2), int(packed), "|", *said]))


def _spread_line(e, n, ran):
    tiles, waves, slots, edge, spec, entries, cap = ran.split("/")
    return " ".join(map(str, ["spread", *e["cells"], *e["support"], e["spread_waves"], slots, cap, n, "|", tiles, waves, edge, spec, *e["tdim"], entries]))


def _rows(golden):
    """The golden file's groups as the program's rows: one per probe call that was recorded."""
    lines = [_gather_line(e["cells"], e["support"], e["options"], e["packed"], e["ran"]) for e in golden["gather_stage_ids"]]
    for e in golden["gather_sweeps"]:
        for pw, planar, packed in zip(e["per_wave"], e["planar"].split(), e["packed"].split()):
            lines.append(_gather_line(e["cells"], e["support"], {"gather_per_wave": pw}, False, planar))
            lines.append(_gather_line(e["cells"], e["support"], {"gather_per_wave": pw}, True, packed))
    for e in golden["gather_options"]:
        lines += [_gather_line(e["cells"], e["support"], e["options"], packed, e[key]) for key, packed in (("planar", False), ("packed", True)) if key in e]
    for e in golden["spread"]:
        off, on = e["slots_off"].split(), e["slots_on"].split()
        for i, n in enumerate(e["N"]):
            lines += [_spread_line(e, n, ran) for ran in [off[i]] + on[2 * i:2 * i + 2]]
    return lines


def test_golden_choices_replayed_on_the_cpu(program):
    """Every row of tests/golden/fcm_launch_choice.json — what uammd_fcm_probe's info said on an MI355X before the choices moved into the
    header: every id of GATHER and SLOT_CASES of tests/test_gpu_fcm_stages.py; the gather at 24^3 for every cubic support 3..13 and every
    (sx, sy, sz) in {5..9}^3, each with gather_per_wave in {-4, -2, -1, 1, 2, 4}, with and without a packed grid, and the three options
    that leave the interleaved gather on the cubic ones; 200^3 and 208^3 either side of the 128 MB bound at supports 5, 6, 7; the spread
    on 24^3, 27^3, 32^3 and 20 x 24 x 28 at supports 4, 6, 9, 13, N either side of 48 and of 64 listed particles, spread_waves 0, 2, 4,
    compact and slot layout — gives the recorded choice."""
    with open(os.path.join(HERE, "golden", "fcm_launch_choice.json")) as fh:
        golden = json.load(fh)
    lines = _rows(golden)
    ids = {e["id"] for e in golden["gather_stage_ids"]} | {e["id"] for e in golden["spread"] if "id" in e}
    assert len(ids) == 38 + 8 and len(lines) == 2522
    out = _run(program, ["replay"], "\n".join(lines) + "\n")
    assert f"replayed {len(lines)} rows: 0 differ" in out


def test_every_input_against_the_kernels_limits(program):
    """Supports 1..16 per axis, cells from {16, 20, 24, 27, 32, 64, 108, 128, 200, 208, 256, 648}, gather_per_wave -4..4, every
    combination of the boolean inputs and of the switches (UAMMD_FCM_GATHER_HALF 0, 1, 2): invariants G1 .. G7, S1 .. S3 and T1 of the
    program hold."""
    out = _run(program, ["enumerate"])
    assert "invariants hold" in out and "BROKEN" not in out
