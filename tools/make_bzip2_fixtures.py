#!/usr/bin/env python3
"""Copy the bzip2 DATA fixtures of the reference's own tests into tests/golden/ref_fixtures/bzip2.

Runs where the reference tree is present.  The inputs are the uuencoded data files next to the reference's tests; they
are decoded to their binary form and written with a manifest of sizes and SHA-256 digests.  The expected payload is what
the reference's read loop gives over the image's libbz2 (tests/bzip2_support.reference_read)."""
import binascii, hashlib, json, os, sys

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "ref_fixtures", "bzip2")
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import bzip2_support as BS      # noqa: E402

FIXTURES = [
    ("cat/test/test_expand.bz2.uu", "cat/test/test_expand_bz2.c"),
    ("libarchive/test/test_compat_bzip2_1.tbz.uu", "test_compat_bzip2.c: 8 concatenated streams"),
    ("libarchive/test/test_compat_bzip2_2.tbz.uu", "test_compat_bzip2.c: a stream and trailing bytes"),
    ("tar/test/test_extract.tar.bz2.uu", "tar/test/test_extract_tar_bz2.c"),
    ("libarchive/test/test_read_format_mtree_crash747.mtree.bz2.uu", "test_read_format_mtree_crash747.c: a damaged stream"),
]


def uudecode(text):
    out = bytearray()
    for line in text.splitlines():
        if line.startswith("begin ") or not line:
            continue
        if line.startswith("end") or line.startswith("`"):
            break
        out += binascii.a2b_uu(line.encode("latin-1"))
    return bytes(out)


def main():
    os.makedirs(OUT, exist_ok=True)
    manifest = []
    for rel, what in FIXTURES:
        raw = uudecode(open(os.path.join(REF, rel), encoding="latin-1").read())
        name = os.path.basename(rel)[:-3]
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(raw)
        data, rc, msg = BS.reference_read(raw)
        manifest.append({"file": name, "source": rel, "what": what, "size": len(raw), "sha256": hashlib.sha256(raw).hexdigest(),
                         "decoded_size": len(data), "decoded_sha256": hashlib.sha256(data).hexdigest(), "rc": rc, "message": msg})
        print(name, len(raw), "->", len(data), rc, msg)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
