"""TEST INFRASTRUCTURE: stage the few files of the reference whose own code the tests run (tests/test_faiss_shim.py, tests/test_rowops.py) into
oracle/_ref/, keeping their paths relative to the reference's root.  oracle/_ref/ is a build product (git-ignored): nothing of the reference is
committed.  The reference checkout is read from $VDK_REFERENCE (default /root/reference); where it is absent or unreadable nothing is staged, and the
tests that execute the reference's code skip with that reason while their committed fixtures (tests/golden/) still run."""
from __future__ import annotations

import os
from pathlib import Path

HERE = Path(__file__).resolve().parent
STAGE = HERE / "_ref"
FILES = ("engine/cbir/evaluation.py", "engine/procedure/train.py", "models/ema.py", "structure/sampler.py")


def reference_root() -> Path:
    return Path(os.environ.get("VDK_REFERENCE", "/root/reference"))


def stage() -> list[str]:
    """copy FILES from the reference into oracle/_ref/; returns the relative paths staged (a file that cannot be read is left out, and a stale copy of it removed)"""
    src = reference_root()
    done = []
    for rel in FILES:
        dst = STAGE / rel
        try:
            data = (src / rel).read_bytes()
        except OSError:
            dst.unlink(missing_ok=True)
            continue
        dst.parent.mkdir(parents=True, exist_ok=True)
        tmp = dst.with_suffix(f".tmp{os.getpid()}")
        tmp.write_bytes(data)
        os.replace(tmp, dst)
        done.append(rel)
    return done


def staged(rel: str) -> Path | None:
    """the staged copy of a reference file, None if build() could not stage it"""
    p = STAGE / rel
    return p if p.is_file() else None


if __name__ == "__main__":
    print(stage())
