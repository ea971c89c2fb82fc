"""The rule of lh264_decode_batch_ex5 (include/lh264.h) restated from two facts of a stream: where its IDR pictures are
(pick (data, "idr")) and how many pictures it has.  Entry pictures are picture 0 and the IDR pictures; a requested picture that exists
needs everything from the last entry at or before it."""


def requested(select, count):
    """the numbers < count that one stream's select= (None | a slice | a sequence of ints) asks for, ascending"""
    if select is None:
        return list(range(count))
    if isinstance(select, slice):
        return list(range(count))[select]
    return [r for r in select if r < count]


def model(idr, count, select):
    """(needed, delivered) for a stream of `count` pictures whose IDR pictures are `idr`"""
    entries = sorted(set([0]) | set(idr))
    delivered = requested(select, count)
    needed = set()
    for r in delivered:
        needed.update(range(max(e for e in entries if e <= r), r + 1))
    return sorted(needed), delivered
