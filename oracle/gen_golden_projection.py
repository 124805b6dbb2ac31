"""
ORACLE / TEST INFRASTRUCTURE ONLY. Golden results of the projection boundary probes (tests/projection_cases.py), produced by the
UNMODIFIED reference function graph_ltpl.helper_funcs.src.get_s_coord.get_s_coord (get_s_coord.py:8-99; pure NumPy + math.atan2, no
shimmed dependency involved):

    python -m oracle.gen_golden_projection       (container only: needs /root/reference)

  tests/golden/projection_probes.npz   results only -- per polyline of projection_cases.lines(), in the order of its probe set: s, the index
                                       pair as the reference returns it (a closed line's idx1 = -1 where Python wraps), and, to notice a
                                       generator that has drifted from the stored results, the probe count and a CRC of the query
                                       coordinates; the numpy version (np.argpartition decides exact d2 ties, and not the same way in
                                       every version).
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_env                                                     # noqa: E402


def query_crc(probes):
    return zlib.crc32(np.ascontiguousarray(probes.qx).tobytes() + np.ascontiguousarray(probes.qy).tobytes())


def main():
    import projection_cases as pc
    gl, _ = ref_env.load_reference()
    get_s_coord = gl.helper_funcs.src.get_s_coord.get_s_coord
    names, counts, crcs, s_all, pair_all = [], [], [], [], []
    for name in pc.lines():
        ps = pc.probe_set(name)
        line, p = ps.line, ps.probes
        ref_line = np.column_stack((line.x, line.y))
        s, pair = np.empty(p.m), np.empty((p.m, 2), np.int16)
        with np.errstate(invalid="ignore", divide="ignore"):
            for i in range(p.m):
                s[i], pair[i] = get_s_coord(ref_line=ref_line, pos=(float(p.qx[i]), float(p.qy[i])), s_array=line.s, closed=line.closed)
        names.append(name); counts.append(p.m); crcs.append(query_crc(p)); s_all.append(s); pair_all.append(pair)
        print("%-28s %6d probes, %d NaN" % (name, p.m, int(np.isnan(s).sum())))
    out = os.path.join(ROOT, "tests", "golden", "projection_probes.npz")
    np.savez_compressed(out, names=np.array(names), counts=np.array(counts, np.int64), crcs=np.array(crcs, np.int64),
                        s=np.concatenate(s_all), pair=np.concatenate(pair_all), numpy_version=np.array(np.__version__))
    print("written %s: %d probes, %d bytes" % (out, int(sum(counts)), os.path.getsize(out)))


if __name__ == "__main__":
    main()
