"""Regenerate refcmdline.json: what the reference's own generated option parser prints for every command line of
tests/test_cli.py::ARGVS (exit code, stdout, stderr with the program's path replaced by PROG).

The parser is built from a reference tree by `make -C oracle ref REFERENCE=<tree>` into oracle/_ref/refcmdline
(see oracle/refcmdline_main.c); the fixture lets tests/test_cli.py pin the command line contract on checkouts that
have no reference tree.

    python tests/golden/make_refcmdline.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_cli as T  # noqa: E402


def main():
    if not os.path.exists(T.REF):
        raise SystemExit(f"{T.REF} not built: make -C oracle ref REFERENCE=<reference tree>")
    out = []
    for argv in T.ARGVS:
        rc, so, se = T.run(T.REF, *argv)
        out.append({"argv": argv, "rc": rc, "stdout": so.decode("utf-8"), "stderr": se.decode("utf-8")})
    with open(os.path.join(HERE, "refcmdline.json"), "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1, ensure_ascii=False)
        fh.write("\n")
    print(f"{len(out)} command lines -> {os.path.join(HERE, 'refcmdline.json')}")


if __name__ == "__main__":
    main()
