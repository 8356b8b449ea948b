"""Extract the reference's BipartitenessCheck golden vectors into tests/golden/bipartiteness_fixtures.json.

Run where a checkout of the reference (Ren91/gelly-streaming) exists:
    python tests/golden/extract_bipartiteness_fixtures.py <reference checkout>
The JSON it writes is committed; no test reads the reference.

It parses DATA out of two of the reference's test sources (read as text):
  - example/test/BipartitenessCheckTest.java:18-35    Bipartite_RESULT, the 6 edges, the 500 ms merge window
  - example/test/NonBipartitnessCheckTest.java:18-35  NonBipartite_RESULT, the 6 edges, the 500 ms merge window
Only inputs and expected outputs are written -- no reference source text.
"""
from __future__ import annotations

import json
import re
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent / "bipartiteness_fixtures.json"
TESTS = "src/test/java/org/apache/flink/graph/streaming/example/test"


def case(path: Path, result_name: str) -> dict:
    t = path.read_text()
    edges = [[int(a), int(b)] for a, b in re.findall(r"new Edge<>\((\d+)L,\s*(\d+)L,\s*NullValue", t)]
    line = "".join(re.findall(r"\"([^\"]*)\"", re.search(result_name + r"\s*=(.*?);", t, re.S).group(1)))
    ms = int(re.search(r"new BipartitenessCheck<[^>]*>\(\(long\)\s*(\d+)\)", t).group(1))
    return {"edges": edges, "merge_window_ms": ms, "expected": line}


def main() -> int:
    if len(sys.argv) != 2:
        print(__doc__)
        return 2
    ref = Path(sys.argv[1]) / TESTS
    fixtures = {
        "source": "Ren91/gelly-streaming test sources (see extract_bipartiteness_fixtures.py docstring)",
        "BipartitenessCheckTest": case(ref / "BipartitenessCheckTest.java", "Bipartite_RESULT"),
        "NonBipartitnessCheckTest": case(ref / "NonBipartitnessCheckTest.java", "NonBipartite_RESULT"),
    }
    OUT.write_text(json.dumps(fixtures, indent=1) + "\n")
    print(f"wrote {OUT}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
