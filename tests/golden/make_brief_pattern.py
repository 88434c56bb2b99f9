"""brief_pattern.npz from the reference's settings file support_files/brief_pattern.yml (four lists of 256 integers):
    python make_brief_pattern.py <path to brief_pattern.yml>
The file holds `x1:`, `y1:`, `x2:`, `y2:` followed by one `  - <int>` line per entry; nothing else is read."""
import os
import sys

import numpy as np


def read(path):
    lists, cur = {}, None
    for line in open(path):
        line = line.strip()
        if line.endswith(":") and line[:-1] in ("x1", "y1", "x2", "y2"):
            cur = lists.setdefault(line[:-1], [])
        elif line.startswith("- ") and cur is not None:
            cur.append(int(line[2:]))
    assert sorted(lists) == ["x1", "x2", "y1", "y2"] and all(len(v) == 256 for v in lists.values())
    return {k: np.asarray(v, np.int32) for k, v in lists.items()}


if __name__ == "__main__":
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "brief_pattern.npz"), **read(sys.argv[1]))
