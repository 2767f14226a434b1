#!/usr/bin/env python3
"""Regenerates tests/golden/reference_java_classes.json: the names of the reference's Java class
files, as package paths (org/apache/bookkeeper/util/ByteBufList.java), from every module's
src/main/java ("main") and src/test/java ("test"). Names only, no source text.
tests/test_java_sources.py resolves the imports of native/java against this list, so that it runs
where the reference tree is absent.

Run where the reference tree exists:  python tests/golden/make_java_index.py [REFERENCE_ROOT]
"""
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_java_classes.json")


def class_files(ref_root: str) -> dict:
    out = {}
    for tree in ("main", "test"):
        marker = os.path.join("src", tree, "java") + os.sep
        names = set()
        for p in glob.glob(os.path.join(ref_root, "**", "src", tree, "java", "**", "*.java"), recursive=True):
            names.add(os.path.relpath(p, ref_root).split(marker, 1)[1].replace(os.sep, "/"))
        out[tree] = sorted(names)
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import oracle
    root = sys.argv[1] if len(sys.argv) > 1 else oracle.REF_ROOT
    if not os.path.isdir(root):
        raise SystemExit(f"reference tree not found at {root}")
    index = class_files(root)
    with open(OUT, "w") as f:
        json.dump(index, f, indent=0)
        f.write("\n")
    print({k: len(v) for k, v in index.items()}, "->", OUT)
