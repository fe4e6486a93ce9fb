"""Drop-in `lib` package: the pieces of the reference's lib/ that sit on the fusion hot path (loss / train step)."""
from immtsf.dropin import extend_package_path as _extend
from immtsf.dropin import overlay_module as _overlay

_extend(__name__, __path__)     # unmirrored modules of the reference keep resolving (immtsf/dropin.py)
# lib.parse_datasets stays the reference's module; its two entry points become the resident loaders' (lib/resident_datasets.py)
_overlay(__name__ + ".parse_datasets", __name__ + ".resident_datasets")
