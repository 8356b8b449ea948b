"""Record what java/patches/*.patch expect of the tree they patch, into tests/golden/patch_preimage.json.

    python tests/golden/extract_patch_preimage.py PATH_TO_THE_GELLY_STREAMING_TREE

For every file a patch touches: the git blob id of the tree's file, its line count, and for every hunk the
sha256 of the tree's own lines at the hunk's position (old start, old count).  tests/test_abi.py compares the
patch's pre-image (context + removed lines) with these digests, i.e. what `git apply --check` would decide in
that tree, without the tree.  Only digests and line numbers are written -- no source text of the tree.
"""
import hashlib
import json
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
OUT = Path(__file__).resolve().parent / "patch_preimage.json"
HUNK = re.compile(r"^@@ -(\d+)(?:,(\d+))? \+\d+(?:,\d+)? @@")


def hunks_of(patch_text):
    """{file: [(old_start, old_count, [pre-image lines])]} of a unified diff."""
    files, cur, body = {}, None, None
    lines = patch_text.split("\n")   # (not splitlines: a patched file with CRLF ends keeps its CRs)
    for line in lines[:-1] if lines[-1] == "" else lines:
        if line.startswith("--- a/"):
            cur = files.setdefault(line[6:], [])
            body = None
        elif (m := HUNK.match(line)) and cur is not None:
            body = []
            cur.append((int(m.group(1)), int(m.group(2) or 1), body))
        elif body is not None and (line[:1] in (" ", "-") or not line):   # ("": an empty context line, stripped)
            body.append(line[1:])
        elif body is not None and line[:1] not in ("+", "\\"):
            body = None   # the next file's header
    return files


def read_patch(path):
    return Path(path).read_bytes().decode()   # (read_text would turn CRLF into LF)


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def main():
    tree = Path(sys.argv[1])
    out = {}
    for patch in sorted((ROOT / "java" / "patches").glob("*.patch")):
        rec = out[patch.name] = {}
        for name, hunks in hunks_of(read_patch(patch)).items():
            data = (tree / name).read_bytes()
            lines = data.decode().split("\n")
            rec[name] = {"blob": hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest(),
                         "hunks": [{"start": s, "count": c, "sha256": digest(lines[s - 1:s - 1 + c])}
                                   for s, c, _ in hunks]}
    OUT.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
