"""Writes tests/golden/optdense_table.json: variable, title, type and first default of every DEFVAR_OPTDENSE_* / MDEFVAR_OPTDENSE_* line of the
reference's libs/MVS/DepthMap.cpp, in order -- the list tests/test_optdense.py checks openmvs_amd.optdense.table() against.

    python tests/golden/make_optdense_golden.py <OpenMVS source tree>
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

if __name__ == "__main__":
    ref = []
    for line in open(os.path.join(sys.argv[1], "libs", "MVS", "DepthMap.cpp"), encoding="utf-8", errors="replace"):
        m = re.match(r'M?DEFVAR_OPTDENSE_(\w+)\((\w+), "([^"]*)", "[^"]*", "([^"]*)"', line)
        if m:
            ref.append((m.group(2), m.group(3), m.group(1), m.group(4)))
    assert len(ref) == 46, len(ref)
    with open(os.path.join(HERE, "optdense_table.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in ref) + "\n]\n")
    print("%d options -> optdense_table.json" % len(ref))
