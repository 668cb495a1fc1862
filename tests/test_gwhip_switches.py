"""The environment switches of the kernel library (genomeworks_amd/csrc/gwhip_switches.h): tests/cpp/switches_driver.cpp
prints what the three readers make of the environment it is started in, and the expectations below are written out by hand
from the parsing rules the launch code has always had (atoi for the integers, the value's first character for the rest).
The driver is built twice, plainly and with the address and undefined-behaviour sanitizers; no GPU is needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "switches_driver.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}

DEFAULTS = {
    "poa": dict(debug_flags=0, persistent_grid=1, msa_serial=0, consensus_hbm_only=0, consensus_full_tables=0),
    "myers": dict(skip=0, hbm_state=0, group=-1, group_lanes=0, mirror_blocks=16),
    "hirschberg": dict(wave=-1, levels=1, span=1, span_single_wave=0),
}

# (environment, what differs from DEFAULTS)
CASES = {
    "unset": ({}, {}),
    "debug_value": ({"GWHIP_DEBUG": "256"}, {"debug_flags": 256}),
    "debug_top_bit_in_use": ({"GWHIP_DEBUG": str(1 << 30)}, {"debug_flags": 1 << 30}),
    "debug_junk": ({"GWHIP_DEBUG": "abc"}, {}),
    "debug_empty": ({"GWHIP_DEBUG": ""}, {}),
    "debug_digits_then_junk": ({"GWHIP_DEBUG": "12abc"}, {"debug_flags": 12}),
    "persistent_off": ({"GWHIP_POA_PERSISTENT": "0"}, {"persistent_grid": 0}),
    "persistent_other": ({"GWHIP_POA_PERSISTENT": "1"}, {}),
    "persistent_first_character_counts": ({"GWHIP_POA_PERSISTENT": "10"}, {}),
    "msa_serial": ({"GWHIP_MSA_SERIAL": "1"}, {"msa_serial": 1}),
    "msa_serial_other": ({"GWHIP_MSA_SERIAL": "0"}, {}),
    "consensus_hbm_only": ({"GWHIP_CONSENSUS_SERIAL": "1"}, {"consensus_hbm_only": 1}),
    "consensus_full_tables": ({"GWHIP_CONSENSUS_SERIAL": "2"}, {"consensus_full_tables": 1}),
    "consensus_other": ({"GWHIP_CONSENSUS_SERIAL": "3"}, {}),
    "myers_skip": ({"GWHIP_MYERS_SKIP": "3"}, {"skip": 3}),
    "myers_hbm_state": ({"GWHIP_MYERS_HBM_STATE": "1"}, {"hbm_state": 1}),
    "myers_group_never": ({"GWHIP_MYERS_GROUP": "0"}, {"group": 0}),
    "myers_group_always": ({"GWHIP_MYERS_GROUP": "1"}, {"group": 1}),
    "myers_group_other": ({"GWHIP_MYERS_GROUP": "2"}, {}),
    "myers_group_lanes_6": ({"GWHIP_MYERS_GROUP_LANES": "6"}, {"group_lanes": 6}),
    "myers_group_lanes_8": ({"GWHIP_MYERS_GROUP_LANES": "8"}, {"group_lanes": 8}),
    "myers_group_lanes_16": ({"GWHIP_MYERS_GROUP_LANES": "16"}, {"group_lanes": 16}),
    "myers_group_lanes_32": ({"GWHIP_MYERS_GROUP_LANES": "32"}, {"group_lanes": 32}),
    "myers_group_lanes_64": ({"GWHIP_MYERS_GROUP_LANES": "64"}, {"group_lanes": 64}),
    "myers_group_lanes_not_a_choice": ({"GWHIP_MYERS_GROUP_LANES": "7"}, {}),
    "mirror_blocks": ({"GWHIP_MIRROR_BLOCKS": "4"}, {"mirror_blocks": 4}),
    "mirror_blocks_at_least_one": ({"GWHIP_MIRROR_BLOCKS": "0"}, {"mirror_blocks": 1}),
    "mirror_blocks_negative": ({"GWHIP_MIRROR_BLOCKS": "-3"}, {"mirror_blocks": 1}),
    "mirror_blocks_empty": ({"GWHIP_MIRROR_BLOCKS": ""}, {"mirror_blocks": 1}),
    "hirschberg_wave_never": ({"GWHIP_HIRSCHBERG_WAVE": "0"}, {"wave": 0}),
    "hirschberg_wave_always": ({"GWHIP_HIRSCHBERG_WAVE": "1"}, {"wave": 1}),
    "hirschberg_levels_off": ({"GWHIP_HIRSCHBERG_LEVELS": "0"}, {"levels": 0}),
    "hirschberg_levels_other": ({"GWHIP_HIRSCHBERG_LEVELS": "1"}, {}),
    "hirschberg_span_off": ({"GWHIP_HIRSCHBERG_SPAN": "0"}, {"span": 0}),
    "hirschberg_span_single_wave": ({"GWHIP_HIRSCHBERG_SPAN": "1"}, {"span_single_wave": 1}),
    "empty_strings": ({name: "" for name in ("GWHIP_POA_PERSISTENT", "GWHIP_MSA_SERIAL", "GWHIP_CONSENSUS_SERIAL", "GWHIP_MYERS_SKIP",
                                             "GWHIP_MYERS_HBM_STATE", "GWHIP_MYERS_GROUP", "GWHIP_MYERS_GROUP_LANES",
                                             "GWHIP_HIRSCHBERG_WAVE", "GWHIP_HIRSCHBERG_LEVELS", "GWHIP_HIRSCHBERG_SPAN")}, {}),
    "several_at_once": ({"GWHIP_DEBUG": "8388608", "GWHIP_CONSENSUS_SERIAL": "1", "GWHIP_MYERS_GROUP": "1", "GWHIP_MYERS_GROUP_LANES": "32",
                         "GWHIP_HIRSCHBERG_SPAN": "1", "GWHIP_HIRSCHBERG_WAVE": "1"},
                        {"debug_flags": 8388608, "consensus_hbm_only": 1, "group": 1, "group_lanes": 32, "span_single_wave": 1, "wave": 1}),
}


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    out = {}
    for name, flags in BUILDS.items():
        exe = str(tmp_path_factory.mktemp("switches") / ("switches_driver_" + name))
        r = subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror"] + flags + [SOURCE, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out[name] = exe
    return out


def expected_lines(changes):
    left = dict(changes)
    lines = []
    for struct, fields in DEFAULTS.items():
        lines.append(" ".join([struct] + ["%s=%d" % (k, left.pop(k, v)) for k, v in fields.items()]))
    assert not left, left  # a misspelt field in the table above
    return lines


@pytest.mark.parametrize("case", sorted(CASES))
def test_readers_parse_the_environment_as_the_launch_code_always_did(drivers, case):
    env_changes, changes = CASES[case]
    env = {k: v for k, v in os.environ.items() if not k.startswith("GWHIP_")}
    env.update(env_changes)
    for build, exe in drivers.items():
        r = subprocess.run([exe], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and r.stderr == "", (build, r.stdout + r.stderr)
        assert r.stdout.splitlines() == expected_lines(changes), (build, case)
