"""
Two-bit nucleotide encoding: the integer keys of :class:`sctools_amd.barcode.Barcodes` and the
codes of the device correction table (``include/sct_barcode.h``) share it.

Same results as the reference's ``sctools.encodings.TwoBit`` (``encodings.py:124-209``):
A=0, C=1, T=2, G=3 in either case, the first base in the highest bits; an IUPAC ambiguity
code becomes a random base (``encodings.py:165-173``); any other byte is a ``KeyError``.
"""
import random

_CODE = {ord("A"): 0, ord("C"): 1, ord("T"): 2, ord("G"): 3, ord("a"): 0, ord("c"): 1, ord("t"): 2, ord("g"): 3}
_AMBIGUOUS = frozenset(ord(c) for c in "MRWSYKVHDBNmrwsykvhdbn")
_BASES = (b"A", b"C", b"T", b"G")


class TwoBit:
    """Fixed-length 2-bit DNA code.  A code does not carry its length (a leading A is 0), so
    decoding and GC content take ``sequence_length`` from the instance."""

    bits_per_base = 2

    def __init__(self, sequence_length: int):
        self.sequence_length = sequence_length

    @classmethod
    def encode(cls, bytes_encoded: bytes) -> int:
        code = 0
        for byte in bytes_encoded:
            base = _CODE.get(byte)
            if base is None:
                if byte not in _AMBIGUOUS:
                    raise KeyError("%s is not a valid IUPAC nucleotide code" % chr(byte))
                base = random.randint(0, 3)
            code = (code << 2) + base
        return code

    def decode(self, integer_encoded: int) -> bytes:
        return b"".join(_BASES[(integer_encoded >> (2 * k)) & 3] for k in reversed(range(self.sequence_length)))

    def gc_content(self, integer_encoded: int) -> int:
        """Number of G or C bases: the two codes with the low bit set."""
        return sum((integer_encoded >> (2 * k)) & 1 for k in range(self.sequence_length))

    @staticmethod
    def hamming_distance(a: int, b: int) -> int:
        """Number of positions at which the two codes hold different bases."""
        d = a ^ b
        d = (d | (d >> 1)) & int("01" * (max(d.bit_length(), 2) // 2 + 1), 2)
        return bin(d).count("1")
