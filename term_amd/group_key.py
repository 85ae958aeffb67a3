"""The canonical bytes of a tuple GROUP BY key (include/tgx.h, TGX_CHECK_GROUP_COUNTS with a column list): what
State.group_counts / State.group_sums hand out as the keys of a task that groups by several columns.

A key is its components one behind the other:

    None    0x00
    int     0x01, then the 8 big-endian bytes of value ^ 2^63 (an int64)
    bytes   0x02, then the length as 2 big-endian bytes, then the bytes (at most 65 535)

The form is prefix-free per component, so it is injective for a given arity, and bytewise ascending order is
lexicographic by component: None before ints before bytes, ints in numeric order, bytes by length and then bytewise."""
import struct

_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1


def encode(cells):
    """the key of the tuple `cells`: each cell None, an int (an int64) or bytes"""
    out = bytearray()
    for c in cells:
        if c is None:
            out.append(0)
        elif isinstance(c, (bytes, bytearray)):
            if len(c) > 0xFFFF:
                raise ValueError("a string component of %d bytes has no encoded form" % len(c))
            out += struct.pack(">BH", 2, len(c)) + bytes(c)
        elif isinstance(c, bool) or not hasattr(c, "__index__"):
            raise TypeError("a cell is None, an int or bytes, not %r" % type(c).__name__)
        else:
            v = int(c)
            if not _I64_MIN <= v <= _I64_MAX:
                raise ValueError("%d is no int64" % v)
            out += struct.pack(">BQ", 1, v + (1 << 63))
    return bytes(out)


def decode(key):
    """the tuple whose key `key` is; ValueError where the bytes are no key"""
    key = bytes(key)
    cells, at, n = [], 0, len(key)
    while at < n:
        tag = key[at]
        at += 1
        if tag == 0:
            cells.append(None)
        elif tag == 1:
            if n - at < 8:
                raise ValueError("an integer component runs past the end of the key")
            cells.append(struct.unpack_from(">Q", key, at)[0] - (1 << 63))
            at += 8
        elif tag == 2:
            if n - at < 2:
                raise ValueError("a string component runs past the end of the key")
            length = struct.unpack_from(">H", key, at)[0]
            at += 2
            if n - at < length:
                raise ValueError("a string component runs past the end of the key")
            cells.append(key[at:at + length])
            at += length
        else:
            raise ValueError("unknown component tag %d" % tag)
    return tuple(cells)
