"""np.savez with LZMA members, for golden files that deflate leaves above the 1 MiB limit of a committed file.
np.load reads the result like any .npz (zipfile decompresses LZMA members transparently)."""
import io
import zipfile

import numpy as np


def savez_lzma(path, **arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))   # no clock: same arrays, same file
            info.compress_type = zipfile.ZIP_LZMA
            info.external_attr = 0o600 << 16
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":   # recompress existing files in place: python tests/golden/npz_lzma.py FILE.npz ...
    import sys
    for f in sys.argv[1:]:
        with np.load(f, allow_pickle=False) as d:
            arrs = {k: d[k] for k in d.files}
        savez_lzma(f, **arrs)
