"""matryodshka_amd -- MI355X (gfx950) native multi-sphere-image infer -> render path.

    from matryodshka_amd import MSI          # needs libmsi_hip.so (python -m matryodshka_amd.build)

The package import itself stays light so that `python -m matryodshka_amd.build`
works before the shared library exists; touching `MSI`, `nets` or `_native`
loads the library and raises if it is missing (there is no CPU fallback).
"""
__version__ = "0.1.0"


def __getattr__(name):
    if name == "MSI":
        from .msi import MSI
        return MSI
    if name == "PackedLayers":      # (packed.py does not load the library: a saved stack can be read on a host without a GPU)
        from .packed import PackedLayers
        return PackedLayers
    if name == "SparseLayers":      # (sparse.py neither)
        from .sparse import SparseLayers
        return SparseLayers
    if name == "FactoredLayers":    # (factored.py neither)
        from .factored import FactoredLayers
        return FactoredLayers
    if name == "MipLayers":         # (mips.py neither)
        from .mips import MipLayers
        return MipLayers
    raise AttributeError(name)
