"""The switches of csrc/ are an explicit, short list: eight runtime knobs
(getenv), the numeric build parameters and the instrumentation.  An A/B loser
is deleted, not left behind as another opt-in (DESIGN.md's "tried" tables keep
the numbers and the commit that last held the code)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phase-based-motion-manipulation_amd", "csrc")

ENV_KNOBS = {"MM_DEBUG", "MM_K2_NOTAB", "MM_K2_TAIL", "MM_K2_TAIL2", "MM_K34_ROWS", "MM_K34_ONESHOT",
             "MM_SB_NF", "MM_SB_CF"}
BUILD_PARAMS = {"MM_K1_GROUPS", "MM_K2_GROUPS", "MM_K3_GROUPS", "MM_Q_TILE_8K", "MM_K2_OPX2G", "MM_K2_WAVES",
                "MM_K4_ROWS", "MM_K4_COLS", "MM_SB_RROWS", "MM_SB_COLS_RUN", "MM_K34_ROWS_4K"}
INSTRUMENTATION = {"MM_K2_STAMPS", "MM_K34_STAMPS", "MM_ASM_MARKS", "MM_ONLY_LOG2N"}


def test_csrc_switches_are_the_listed_ones():
    env, pre = set(), set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")):
        for line in open(path):
            env.update(re.findall(r'getenv\("(MM_\w+)"\)', line))
            if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                pre.update(re.findall(r"\bMM_\w+", line))
    assert env == ENV_KNOBS
    assert pre == BUILD_PARAMS | INSTRUMENTATION
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert not [k for k in ENV_KNOBS if k not in design]
