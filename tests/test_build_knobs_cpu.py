"""DESIGN.md's "Build-time knobs" table lists exactly the SMX_ macros that preprocessor conditionals of csrc/ test.

Source text only: nothing is compiled.  A switch added to a header without a line in the table, or a line whose macro no
conditional tests any more, fails here.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def conditional_macros():
    found = set()
    for path in glob.glob(os.path.join(ROOT, "stereo-depth_amd", "csrc", "*.*")):
        text = open(path, encoding="utf-8").read().replace("\\\n", " ")
        for cond in re.findall(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", text, re.M):
            found |= set(re.findall(r"\bSMX_\w+", cond.split("//")[0]))
    return found


def listed_macros():
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    after = text.split("**Build-time knobs.**", 1)[1]
    table = re.search(r"(?:^\|.*\n)+", after, re.M).group(0)
    return set(re.findall(r"^\| `(SMX_\w+)` \|", table, re.M))


def test_build_knobs_table_matches_the_sources():
    tested, listed = conditional_macros(), listed_macros()
    assert listed, "DESIGN.md: the Build-time knobs table is empty or missing"
    assert tested - listed == set(), f"tested in csrc/ but not in DESIGN.md's table: {sorted(tested - listed)}"
    assert listed - tested == set(), f"in DESIGN.md's table but tested nowhere in csrc/: {sorted(listed - tested)}"
