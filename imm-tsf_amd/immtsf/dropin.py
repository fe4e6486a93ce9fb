"""How the mirrored packages coexist with the reference tree they are dropped in front of.

`imm-tsf_amd/` goes FIRST on sys.path and ships packages with the reference's names (`fusions`, `layers`, `models`,
`lib`).  A regular package would hide the reference's directory of the same name, and with it every module this build
does not mirror (`lib.utils`, `lib.parse_datasets`, `layers.Attn_Bias`, ...), so:

  * `extend_package_path` (called from each package's __init__) appends the same-named directories found further along
    sys.path to the package's __path__: mirrored modules resolve here, everything else resolves to the reference;
  * `reexport_missing` (called at the end of a mirrored module) loads the shadowed reference module of the same name, if
    one exists, and copies the public names this build does not define (`layers.Embed.DataEmbedding_wo_pos`,
    `layers.Transformer_EncDec.TimerLayer`, ...), so the reference's other models keep importing what they need.

  * `overlay_module` (called from a package's __init__) is for a module of the reference that stays the reference's -- its file, its
    names -- while this build replaces some of its entry points: when `<package>.<leaf>` is imported, the reference's module further
    along the package's __path__ is executed as usual and then handed to `install(module)` of the module here that carries the
    replacements (`lib.parse_datasets`: the reference's module with `parse_datasets` / `get_input_and_pred_len` of
    `lib.resident_datasets` installed; `models.Informer`: the reference's module with the `Informer` class of `models.informer_model`
    installed when what it finds there is the reference's model).  With no such module on the path the name is an alias of the module here, so it imports
    standalone too.  Why not a mirrored file lib/parse_datasets.py ending in reexport_missing, like the others:
    tests/test_dropin_packages.py::test_reference_main_imports_resolve_with_this_tree_in_front pins `lib.parse_datasets.__file__` to the
    tree behind this one, and a file of that name here would always be found first.

The first two are no-ops when no reference tree is on the path (the tests, the GPU box).
"""
from __future__ import annotations

import importlib
import importlib.abc
import importlib.machinery
import importlib.util
import os
import sys


def extend_package_path(name: str, path: list) -> None:
    own = {os.path.realpath(p) for p in path}
    for entry in sys.path:
        cand = os.path.join(entry or ".", *name.split("."))
        if os.path.isdir(cand) and os.path.realpath(cand) not in own:
            path.append(cand)
            own.add(os.path.realpath(cand))


def reexport_missing(module_globals: dict) -> None:
    mod_name, mod_file = module_globals["__name__"], module_globals.get("__file__")
    if not mod_file or "." not in mod_name:
        return
    pkg_name, leaf = mod_name.rsplit(".", 1)
    pkg = sys.modules.get(pkg_name)
    if pkg is None:
        return
    for d in list(getattr(pkg, "__path__", [])):
        cand = os.path.join(d, leaf + ".py")
        if os.path.isfile(cand) and os.path.realpath(cand) != os.path.realpath(mod_file):
            alias = f"{pkg_name}._shadowed_{leaf}"
            if alias in sys.modules:
                other = sys.modules[alias]
            else:
                spec = importlib.util.spec_from_file_location(alias, cand)
                other = importlib.util.module_from_spec(spec)
                sys.modules[alias] = other
                try:
                    spec.loader.exec_module(other)
                except Exception:          # a dependency of the shadowed module is missing: nothing to re-export
                    sys.modules.pop(alias, None)
                    return
            for k, v in vars(other).items():
                if not k.startswith("_") and k not in module_globals:
                    module_globals[k] = v
            return


class _Alias(importlib.abc.Loader):
    """`fullname` is the already importable module `target`, the same object under a second name"""

    def __init__(self, target):
        self.target = target

    def create_module(self, spec):
        return importlib.import_module(self.target)

    def exec_module(self, module):
        pass


class _Overlay(importlib.abc.MetaPathFinder):
    def __init__(self, fullname, target):
        self.fullname, self.target = fullname, target

    def find_spec(self, fullname, path=None, target=None):
        if fullname != self.fullname:
            return None
        spec = importlib.machinery.PathFinder.find_spec(fullname, path)
        if spec is None or spec.loader is None:         # nothing behind this tree: the module here under the reference's name
            return importlib.machinery.ModuleSpec(fullname, _Alias(self.target), origin=importlib.util.find_spec(self.target).origin)
        inner, target = spec.loader, self.target

        class Loader(importlib.abc.Loader):
            def create_module(self, spec):
                return inner.create_module(spec)

            def exec_module(self, module):
                inner.exec_module(module)
                importlib.import_module(target).install(module)

            def __getattr__(self, name):        # get_code, get_source, get_filename, ...: the file loader's own
                return getattr(inner, name)

        spec.loader = Loader()
        return spec


def overlay_module(fullname: str, target: str) -> None:
    if not any(isinstance(f, _Overlay) and f.fullname == fullname for f in sys.meta_path):
        sys.meta_path.insert(0, _Overlay(fullname, target))


# ---- torch.autocast around the drop-in entry points -------------------------------------------------------------------------------
# main.py --use_amp runs the step inside `autocast()` (main.py:1080-1091).  This build's precision is immtsf.config.precision's: its
# kernels take fp32 tensors and choose their own MFMA operands, and it has no fp16 path.  Autocast would only reach the torch ops
# BETWEEN the kernels (an fp16 linear here, a bf16 matmul there) and feed half tensors into autograd Functions that expect fp32, so the
# entry points compute under autocast exactly what they compute outside it.

def _to_fp32(x):
    import torch
    if torch.is_tensor(x):
        return x.float() if x.dtype in (torch.float16, torch.bfloat16) else x
    if isinstance(x, dict):
        return {k: _to_fp32(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_to_fp32(v) for v in x)
    return x


def fp32_entry(fn):
    """decorator of a drop-in entry point (lib.evaluation.compute_all_losses / evaluation, FusionModel.forward, <backbone>.forecasting):
    inside torch.autocast the call runs with autocast disabled and half tensors among its arguments widened to fp32; outside it the
    call is fn's own, untouched"""
    import functools

    @functools.wraps(fn)
    def entry(*args, **kwargs):
        import torch
        if not torch.is_autocast_enabled("cuda"):
            return fn(*args, **kwargs)
        with torch.autocast("cuda", enabled=False):
            return fn(*_to_fp32(args), **_to_fp32(kwargs))
    return entry
