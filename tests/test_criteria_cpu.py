"""CPU: the host front end that the four criteria share (lm_net_amd.loss: BoundaryLoss, HausdorffDTLoss, LovaszLoss, RegionLoss and
the functions lovasz_ranks, region_sums, distance_maps): every rule on the class count, the class list, the head, the logits and the
target is refused with the same words by every criterion, and no criterion keeps its scratch where torch.nn.Module keeps its
registries.  The rules of one family alone (limits, kinds, denominators, "present", alpha) are in that family's own file.  No GPU needed."""
import pytest
import torch

from lm_net_amd import BoundaryLoss, HausdorffDTLoss, LovaszLoss, RegionLoss, distance_maps, lovasz_ranks, region_sums

CRITERIA = [BoundaryLoss, HausdorffDTLoss, LovaszLoss, RegionLoss]
FUNCTIONS = [lovasz_ranks, region_sums]
Y = torch.zeros(2, 8, 9, dtype=torch.int64)
Z = torch.zeros(2, 3, 8, 9)


def _make(target, n_classes, **kw):
    """A criterion or a function as f(logits, target); a function checks its configuration when it is called."""
    if isinstance(target, type):
        return target(n_classes, **kw)
    return lambda logits, labels: target(logits, labels, n_classes, **kw)


def _configure(target, n_classes, **kw):
    f = _make(target, n_classes, **kw)
    if not isinstance(target, type):
        f(Z, Y)


CONFIG_ROWS = [(dict(n_classes=0), "n_classes"), (dict(n_classes=65), "n_classes"), (dict(n_classes=3, head="tanh"), "head"),
               (dict(n_classes=3, head="tanh"), "expected 'softmax' or 'sigmoid'"), (dict(n_classes=1), "head='sigmoid'"),
               (dict(n_classes=3, classes=[0, 0]), "distinct"), (dict(n_classes=3, classes=[5]), "distinct"), (dict(n_classes=3, classes=[]), "distinct"),
               (dict(n_classes=3, classes=[1.5]), "distinct")]


@pytest.mark.parametrize("target", CRITERIA + FUNCTIONS, ids=lambda t: t.__name__)
def test_configuration_is_refused_in_one_voice(target):
    for kw, msg in CONFIG_ROWS:
        with pytest.raises(ValueError, match="%s: .*%s" % (target.__name__, msg)):
            _configure(target, **kw)


def test_distance_maps_takes_the_same_class_rules():
    """distance_maps has a mode where the criteria have a head; the class count and the class list are the shared parser's."""
    for args, kw in (((Y, 0), {}), ((Y, 65), {})):
        with pytest.raises(ValueError, match="distance_maps: n_classes"):
            distance_maps(*args, **kw)
    for classes in ([1, 1], [0, 0], [3], [5], [], [1.5]):
        with pytest.raises(ValueError, match="distance_maps: .*distinct"):
            distance_maps(Y, 3, classes=classes)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        distance_maps(Y, 3)


PAIR_ROWS = [((Z[:, :2], Y), "logits must be"), ((Z[0], Y), "logits must be"), ((Z, Y[:, :4]), "does not match"), ((Z, Y.float()), "uint8, bool or int64"),
             ((Z, torch.zeros(2, 3, 8, 9, dtype=torch.int64)), "does not match")]          # the last: planes under a softmax head


@pytest.mark.parametrize("target", CRITERIA + FUNCTIONS, ids=lambda t: t.__name__)
def test_logits_and_target_are_checked_in_one_voice(target):
    f = _make(target, 3)
    for args, msg in PAIR_ROWS:
        with pytest.raises(ValueError, match="%s: .*%s" % (target.__name__, msg)):
            f(*args)
    with pytest.raises(ValueError, match="does not match .* under a sigmoid head"):
        _make(target, 3, head="sigmoid")(Z, Y)                           # a sigmoid head takes planes, not a label map
    with pytest.raises(RuntimeError, match=r"lm_net_amd\.%s: .*no CPU fallback" % target.__name__):
        f(Z, Y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(Z, Y[:, None])                                                 # [B, 1, H, W] labels are taken under a softmax head
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _make(target, 1, head="sigmoid")(Z[:, :1], Y.to(torch.uint8))    # one logit: [B, H, W] planes are taken
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _make(target, 3, head="sigmoid")(Z, torch.zeros(2, 3, 8, 9, dtype=torch.bool))


def test_float_logits_switch():
    """The Lovasz and region front ends refuse integer logits; the distance losses convert them, as they always did."""
    zi = torch.zeros(2, 3, 8, 9, dtype=torch.int32)
    for target in (LovaszLoss, RegionLoss, lovasz_ranks, region_sums):
        with pytest.raises(ValueError, match="logits must be floating point"):
            _make(target, 3)(zi, Y)
    for target in (BoundaryLoss, HausdorffDTLoss):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _make(target, 3)(zi, Y)


@pytest.mark.parametrize("cls", CRITERIA, ids=lambda t: t.__name__)
def test_scale_must_be_finite(cls):
    crit = cls(3)
    for bad in (float("inf"), float("-inf"), float("nan")):
        crit.scale = bad
        with pytest.raises(ValueError, match="%s: scale = .* is not finite" % cls.__name__):
            crit(Z, Y)


# ---------------------------------------------------------------- the scratch and torch.nn.Module's registries
REGISTRIES = ("_parameters", "_buffers", "_modules")


def _fill_as_forward_does(crit):
    """What forward leaves on the module, stored the way forward stores it; the names it used."""
    scratch = (torch.zeros(16, dtype=torch.uint8), torch.zeros(3, 4), torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32))
    if isinstance(crit, (BoundaryLoss, HausdorffDTLoss)):                # no cache: the last maps are plain attributes
        crit.maps = scratch[2]
        if isinstance(crit, HausdorffDTLoss):
            crit.pred_maps = scratch[2].clone()
        return ["maps", "pred_maps"]
    assert crit._scratch == {}
    crit._scratch[(torch.device("cpu"), 2, 8, 9)] = scratch
    if isinstance(crit, LovaszLoss):
        crit.ranks = scratch[1:]
    else:
        crit.sums, crit.counts, crit.per_class = scratch[1:]
    return ["_scratch"]


@pytest.mark.parametrize("cls", CRITERIA, ids=lambda t: t.__name__)
def test_scratch_stays_out_of_the_module_registries(cls):
    """LovaszLoss once kept its scratch in `_buffers`, torch.nn.Module's own buffer registry: after the first forward state_dict() and
    .to() raised on the tuple stored there, in the criterion and in every module that held it."""
    kw = dict(weight=[1.0, 2.0, 3.0]) if cls is RegionLoss else {}
    registered = ["weight"] if cls is RegionLoss else []
    crit = cls(3, **kw)
    assert isinstance(crit._buffers, dict) and all(v is None or isinstance(v, torch.Tensor) for v in crit._buffers.values())
    crit.register_buffer("probe", torch.zeros(1))
    assert sorted(crit.state_dict()) == sorted(registered + ["probe"])
    names = _fill_as_forward_does(crit)
    assert not set(names) & set(REGISTRIES)
    for name in REGISTRIES:
        assert all(v is None or isinstance(v, (torch.Tensor, torch.nn.Module)) for v in getattr(crit, name).values()), name
    assert sorted(crit.state_dict()) == sorted(registered + ["probe"])
    assert sorted(torch.nn.Sequential(crit).state_dict()) == sorted("0." + k for k in registered + ["probe"])
    moved = crit.to(torch.float64)
    assert moved is crit and crit.probe.dtype == torch.float64
    for name in names:                                                   # .to() converts what is registered and nothing else
        held = getattr(crit, name, None)
        for t in ([held] if isinstance(held, torch.Tensor) else [t for v in (held or {}).values() for t in v]):
            assert t.dtype != torch.float64
    assert sorted(crit.state_dict()) == sorted(registered + ["probe"])
