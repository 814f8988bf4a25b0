"""Record what tests/test_citations.py needs to know about the reference sources, so the test runs
without them: tests/golden/reference_lines.json holds the line count of every cited file and, for each
(file, line, text) anchor of the test, a digest written only after `text` was found on that line.
No reference text is stored. usage: python oracle/gen_reference_lines.py REFERENCE_SRC_DIR"""
from __future__ import annotations

import importlib.util
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def main(src: str) -> None:
    spec = importlib.util.spec_from_file_location("test_citations", ROOT / "tests" / "test_citations.py")
    tc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tc)
    lines = {n: (Path(src) / f"{n}.py").read_text().splitlines() for n in tc.FILES}
    anchors = {}
    for name, line, text in tc.ANCHORS:
        if text not in lines[name][line - 1]:
            raise SystemExit(f"{name}.py:{line} does not contain {text!r}")
        anchors[f"{name}:{line}"] = tc.anchor_digest(name, line, text)
    out = {"line_counts": {n: len(v) for n, v in lines.items()}, "anchors_verified": anchors}
    (ROOT / "tests" / "golden" / "reference_lines.json").write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main(sys.argv[1])
