"""What the ``test_*_surface.py`` files share: a library's exported symbols, a header's parsed declarations, tools/kernel_resources.py."""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exported_symbols(path):
    """Names the shared library DEFINES in its dynamic symbol table (ELF64, little endian), read with ``struct``."""
    data = open(path, "rb").read()
    assert data[:6] == b"\x7fELF\x02\x01", "an ELF64 little-endian file"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for s in sections:
        if s[1] != 11:      # SHT_DYNSYM
            continue
        stroff = sections[s[6]][4]
        for off in range(s[4], s[4] + s[5], 24):
            st_name, _info, _other, shndx = struct.unpack_from("<IBBH", data, off)
            if shndx != 0 and st_name:
                end = data.index(b"\0", stroff + st_name)
                names.add(data[stroff + st_name:end].decode())
    return names


def header(name):
    """``include/<name>`` -> (signatures, streamed) as ``_lib.parse_header`` gives them."""
    from driving_dirty_amd import _lib
    return _lib.parse_header(open(os.path.join(ROOT, "include", name)).read())


def kernel_resources():
    """The module tools/kernel_resources.py."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    return kernel_resources
