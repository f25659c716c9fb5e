"""Regenerate qingdai_amd/data/stateframe_cmaps.json: the 256 x 3 f64 lookup tables of the colormaps the reference's plot_state names
(scripts/run_simulation.py:355-499) and, last, the one more its plot_ecology names (:1009), read from the local matplotlib.  The state frame (qingdai_amd/stateframe.py) looks its band
colours up in these tables, so that no matplotlib is needed at run time.  The file is text: every number is written with repr,
which reads back to the same double."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "qingdai_amd", "data", "stateframe_cmaps.json")
NAMES = ("coolwarm", "viridis", "Blues", "Greys", "RdBu_r", "PuOr", "magma", "cividis", "plasma", "GnBu", "YlGn", "BuPu",
         "Greens")      # plot_ecology's canopy-height tile (:1009, qingdai_amd/figures.py)


def main():
    import matplotlib
    tables = {}
    for name in NAMES:
        cm = matplotlib.colormaps[name]
        assert cm.N == 256
        lut = np.asarray(cm(np.arange(256)), dtype=np.float64)[:, :3]      # integer input indexes the table directly
        assert lut.shape == (256, 3) and np.array_equal(lut[-1], np.asarray(cm(2.0))[:3])      # over = the last entry
        tables[name] = np.ascontiguousarray(lut)
    with open(OUT, "w", encoding="ascii") as f:
        f.write("{\n" + ",\n".join(json.dumps(name) + ": [" + ",\n ".join(json.dumps([float(x) for x in row]) for row in t) + "]"
                                  for name, t in tables.items()) + "\n}\n")
    with open(OUT, encoding="ascii") as f:
        back = json.load(f)
    assert all(np.array_equal(np.array(back[name], dtype=np.float64), t) for name, t in tables.items())
    print(f"{os.path.relpath(OUT)}: {len(tables)} tables, {os.path.getsize(OUT)} bytes (matplotlib {matplotlib.__version__})")


if __name__ == "__main__":
    main()
