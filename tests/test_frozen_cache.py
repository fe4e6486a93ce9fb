"""The cache helper of the frozen-LLM drivers (immtsf.ops._frozen_cached) alone, on CPU tensors: no GPU, no library load.  `build` counts
its calls; the images (which need a kernel) are not asked for."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "imm-tsf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


class _Build:
    def __init__(self, *params):
        self.params, self.calls = params, 0

    def __call__(self):
        self.calls += 1
        return (torch.cat([p.detach() for p in self.params], 0).contiguous(),)


def _setup():
    model, owner = torch.nn.Module(), torch.nn.Module()
    a, b = torch.nn.Parameter(torch.randn(3, 4)), torch.nn.Parameter(torch.randn(2, 4))
    return model, owner, a, b


def test_a_hit_builds_nothing_and_returns_the_same_entry():
    from immtsf import ops
    model, owner, a, b = _setup()
    build = _Build(a, b)
    hit = ops._frozen_cached(model, owner, "ab", (a, b), build)
    assert build.calls == 1 and torch.equal(hit.w, torch.cat([a, b], 0).detach()) and hit.items[0] is hit.w
    assert hit.w16 is None and hit.split is None and hit.image(False, False) is None
    for _ in range(3):
        assert ops._frozen_cached(model, owner, "ab", (a, b), build) is hit
    assert build.calls == 1


def test_a_version_bump_with_the_same_data_rebuilds():
    from immtsf import ops
    model, owner, a, b = _setup()
    build = _Build(a, b)
    hit = ops._frozen_cached(model, owner, "ab", (a, b), build)
    ptrs = (a.data_ptr(), b.data_ptr())
    with torch.no_grad():
        b.add_(0)                                         # the second parameter: every parameter is in the key
    assert (a.data_ptr(), b.data_ptr()) == ptrs
    again = ops._frozen_cached(model, owner, "ab", (a, b), build)
    assert build.calls == 2 and again is not hit and torch.equal(again.w, hit.w)
    assert ops._frozen_cached(model, owner, "ab", (a, b), build) is again and build.calls == 2
    with torch.no_grad():
        a.data = a.data.clone()                           # new storage, as .to() or load_state_dict(assign=True) leave it
    assert ops._frozen_cached(model, owner, "ab", (a, b), build) is not again and build.calls == 3


def test_two_slots_under_one_owner_do_not_collide():
    from immtsf import ops
    model, owner, a, b = _setup()
    build_a, build_b = _Build(a), _Build(b)
    hit_a = ops._frozen_cached(model, owner, "a", (a,), build_a)
    hit_b = ops._frozen_cached(model, owner, "b", (b,), build_b)
    assert hit_a is not hit_b and torch.equal(hit_a.w, a.detach()) and torch.equal(hit_b.w, b.detach())
    assert ops._frozen_cached(model, owner, "a", (a,), build_a) is hit_a and ops._frozen_cached(model, owner, "b", (b,), build_b) is hit_b
    assert (build_a.calls, build_b.calls) == (1, 1)
    other = torch.nn.Module()                             # and the same slot under another owner is another entry
    assert ops._frozen_cached(model, other, "a", (a,), build_a) is not hit_a and build_a.calls == 2


def test_two_models_do_not_share_entries():
    from immtsf import ops
    model, owner, a, b = _setup()
    model2 = torch.nn.Module()
    build = _Build(a, b)
    hit = ops._frozen_cached(model, owner, "ab", (a, b), build)
    hit2 = ops._frozen_cached(model2, owner, "ab", (a, b), build)
    assert hit2 is not hit and build.calls == 2
    assert ops._frozen_cached(model, owner, "ab", (a, b), build) is hit and ops._frozen_cached(model2, owner, "ab", (a, b), build) is hit2
    assert build.calls == 2
    assert not any(isinstance(v, dict) and v and all(isinstance(e, ops._FrozenEntry) for e in v.values()) for v in owner.__dict__.values())
