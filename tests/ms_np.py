"""numpy restatement of multi-stream decoding (asr/gaussian/distribBasic.h:135-158, 390-408; distribBasic.cc:326-417): the combination of two score
matrices, the name resolution of the DistribSetMultiStream constructors and the DistribMap file format."""
import struct

import numpy as np

E_INDEX, E_KEY = 6, 11
MAX_NAME = 19                                             # the reference reads names into char[20] (distribBasic.cc:338-339)


class MsError(Exception):
    def __init__(self, status, msg):
        Exception.__init__(self, msg); self.status = status


def combine(sA, sV, table, wA, wV):
    """DistribMultiStream::_score (distribBasic.h:148-152) for every (frame, state): two fp64 products, one fp64 sum, one rounding to float.  numpy
    evaluates the three operations one after the other, each rounded: nothing is fused."""
    return (np.float64(wA) * sA.astype(np.float64) + np.float64(wV) * sV[:, table].astype(np.float64)).astype(np.float32)


def resolve(namesA, namesV, mapping=None):
    """the [KA] table of video state indices (distribBasic.cc:385-391, 400-409): jindex_error for a name the map lacks, jkey_error for a name the
    video set lacks"""
    first = {}
    for i, n in enumerate(namesV):
        first.setdefault(n, i)
    table = np.zeros(len(namesA), np.int32)
    for k, name in enumerate(namesA):
        partner = name
        if mapping is not None:
            if name not in mapping:
                raise MsError(E_INDEX, "No mapping for %s" % name)
            partner = mapping[name]
        if partner not in first:
            raise MsError(E_KEY, "Could not find key %s" % partner)
        table[k] = first[partner]
    return table


def _wstr(s):
    b = s.encode()
    return struct.pack(">h", len(b)) + b + b"\0"           # write_string (mach_ind_io.cc:1009-1021): length, then length + 1 bytes


def distribmap_bytes(mapping):
    """DistribMap::write (distribBasic.cc:359-376): a big-endian int32 count, the pairs in std::map key order (byte-wise)"""
    out = struct.pack(">i", len(mapping))
    for k in sorted(mapping, key=lambda s: s.encode()):
        out += _wstr(k) + _wstr(mapping[k])
    return out


def parse_distribmap(data):
    """DistribMap::read (distribBasic.cc:326-347) -> dict"""
    (n,) = struct.unpack_from(">i", data, 0); pos = 4; out = {}

    def rstr():
        nonlocal pos
        (ln,) = struct.unpack_from(">h", data, pos); pos += 2
        s = data[pos:pos + ln]; assert data[pos + ln:pos + ln + 1] == b"\0"; pos += ln + 1
        return s.decode()
    for _ in range(n):
        k = rstr(); out[k] = rstr()
    assert pos == len(data)
    return out
