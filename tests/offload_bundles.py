"""The clang offload bundles of a HIP library, read without a GPU: a fat binary holds one bundle per translation unit, and each bundle one entry per target.
The library's own AQL loader (csrc/srbdqp_aql.hpp) reads the gfx950 entry of the FIRST bundle the same way."""
import re
import struct

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def gfx950_entry(blob, at):
    """The gfx950 code object of the bundle whose magic stands at blob[at:], or None where the magic is not a bundle's (the loader's own copy of the string)."""
    (n,) = struct.unpack_from("<Q", blob, at + 24)
    pos = at + 32
    if not 1 <= n <= 16:
        return None
    for _ in range(n):
        off, size, tl = struct.unpack_from("<QQQ", blob, pos)
        if tl > 256 or at + off + size > len(blob):
            return None
        triple = blob[pos + 24:pos + 24 + tl]
        pos += 24 + tl
        if b"gfx950" in triple and size > 0:
            return blob[at + off:at + off + size]
    return None


def gfx950_objects(blob):
    """The gfx950 code objects of the offload bundles in a library's bytes, in file order."""
    return [o for o in (gfx950_entry(blob, m.start()) for m in re.finditer(re.escape(MAGIC), blob)) if o is not None]
