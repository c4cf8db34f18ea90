"""The capacities of the LDS match array, read from the sources (registration_dev.h: match_lds_cap(cost) = 8 x CFEAR_MATCH_LDS_CAP / {8, 7, 5}
for P2D, P2L, P2P - match_lds_arrays), per translation unit that compiles the registration, and the number of threads that evaluate
(min(CFEAR_REG_BLOCK, 64 x CFEAR_EVAL_WAVES): the stride of evaluate_partial_t's pair loop). One copy for the tests that place a problem
against a capacity: test_match_capacity_gpu.py, test_surface_paths_gpu.py, test_tc_gpu.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cfear_radarodometry_code_public_amd", "csrc")
P2P, P2L, P2D = 0, 1, 2
COST_NAME = {P2P: "P2P", P2L: "P2L", P2D: "P2D"}


def _define(header, name):
    m = re.search(r"^#define\s+%s\s+(\d+)\s*(?://.*)?$" % name, open(os.path.join(CSRC, header)).read(), re.M)
    assert m, name
    return int(m.group(1))


def caps_of(match_lds_cap):
    """match_lds_cap(cost) of registration_dev.h for one value of CFEAR_MATCH_LDS_CAP -> {cost: residual blocks kept in LDS}"""
    doubles = 8 * match_lds_cap
    return {P2D: doubles // 8, P2L: doubles // 7, P2P: doubles // 5}


# the kernels of the per-call entries (percall.hip) and the 64-scan step kernels (pipeline.hip compiles registration_dev.h with its default)
LDS_CAP = caps_of(_define("registration_dev.h", "CFEAR_MATCH_LDS_CAP"))
REG_BLOCK = _define("registration_dev.h", "CFEAR_REG_BLOCK")  # BLOCK_R: one block of source cells (association path 1)
# instantiation -> ({cost: capacity}, threads that evaluate). (register_step_large.hip has a second value for its two-workgroup A/B
# build; _define takes the first, the one CFEAR_LARGE_WG_PER_CU == 1 compiles)
EVAL_WAVES = _define("registration_dev.h", "CFEAR_EVAL_WAVES")
LARGE_BLOCK = _define("register_step_large.hip", "CFEAR_LARGE_BLOCK")  # its CFEAR_REG_BLOCK, and all of its waves evaluate (CFEAR_LARGE_BLOCK / 64)
INSTANTIATIONS = {
    "pipeline": (LDS_CAP, min(REG_BLOCK, 64 * EVAL_WAVES)),
    "register_step": (caps_of(_define("register_step.hip", "CFEAR_MATCH_LDS_CAP")), min(REG_BLOCK, 64 * EVAL_WAVES)),
    "replay": (caps_of(_define("replay.hip", "CFEAR_MATCH_LDS_CAP")), min(_define("replay.hip", "CFEAR_REG_BLOCK"), 64 * EVAL_WAVES)),
    "register_step_large": (caps_of(_define("register_step_large.hip", "CFEAR_MATCH_LDS_CAP")), LARGE_BLOCK),
}
# the table pinned: a change of a capacity moves the seam, and the cases of test_match_capacity_gpu.py with it. (replay.hip's workgroup
# has 512 threads, but waves 4 .. 7 sit out the evaluations: its pair loop strides by 256. Its trip cases run at both values.)
TABLE = {
    "pipeline": ({P2D: 622, P2L: 710, P2P: 995}, 256),
    "register_step": ({P2D: 784, P2L: 896, P2P: 1254}, 256),
    "replay": ({P2D: 1200, P2L: 1371, P2P: 1920}, 256),
    "register_step_large": ({P2D: 2250, P2L: 2571, P2P: 3600}, 512),
}
