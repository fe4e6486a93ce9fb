"""Drop-in `models` package (same import paths and Model(args).forecasting(...) signatures as the reference)."""
from immtsf.dropin import extend_package_path as _extend
from immtsf.dropin import overlay_module as _overlay

_extend(__name__, __path__)     # unmirrored modules of the reference keep resolving (immtsf/dropin.py)
# models.Informer stays the module of a tree behind this one when there is one, with this build's class installed over the reference's
# (models/informer_model.py); with nothing behind, the name is that module
_overlay(__name__ + ".Informer", __name__ + ".informer_model")
