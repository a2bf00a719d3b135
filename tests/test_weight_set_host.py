"""CPU-side tests of the weight-set protocol `BatchedActor`, `BatchedCritic` and `BatchedTwinCritic` share
(`ris_vec_marl_amd/_weights.py`): taking weights by copy and by reference, the blend's refusals, and the staleness state
that decides whether a kernel's weight stream is rebuilt.  The objects are built without a device (`__new__`, as
test_sarl_critic_pack_host.bare does): every check comes before any use of one.

`load_state_dict` copies and converts, so of the bad tensors below it refuses the wrong shape and the missing key only;
a float64 tensor and a non-contiguous view are taken and converted, and that is asserted too."""
import pytest
import torch

from ris_vec_marl_amd import actor as ACT
from ris_vec_marl_amd import critic as CR
from ris_vec_marl_amd import marl_critic as MC
from tests.test_sarl_critic_pack_host import ACTOR_DIMS, CRITIC_DIMS, bare

TWIN_DIMS = dict(W1=(64, 48), b1=(64,), W2=(128, 64), b2=(128,), W3=(128, 128), b3=(128,), Wq=(1, 128), bq=(1,))
CASES = [pytest.param(ACT.BatchedActor, ACTOR_DIMS, 1, id="actor"), pytest.param(CR.BatchedCritic, CRITIC_DIMS, 1, id="critic"),
         pytest.param(MC.BatchedTwinCritic, TWIN_DIMS, 1, id="twin-1"), pytest.param(MC.BatchedTwinCritic, TWIN_DIMS, 2, id="twin-2")]
WIDE = "fc2.weight"                                           # a 2-d weight of every class, packed into its stream
METHODS = ("load_state_dict", "share_state_dict", "soft_update_from")


class Subject:
    """One object under test and its weight sets: itself, or the nets of a twin critic."""

    def __init__(self, cls, dims, n_nets, device="cpu"):
        self.twin = cls is MC.BatchedTwinCritic
        if self.twin:
            self.obj = cls.__new__(cls)
            self.obj.device, self.obj.n_nets, self.obj.packs = torch.device(device), n_nets, 0
            self.obj.nets = [bare(MC._Net, dims, device) for _ in range(n_nets)]
        else:
            self.obj = bare(cls, dims, device)
        self.sets = self.obj.nets if self.twin else [self.obj]
        self.dims, self.sd_keys = dims, self.sets[0]._SD
        self.kept = [{a: getattr(ws, a) for a in dims} for ws in self.sets]

    def mappings(self, fill=1.0):
        return [{k: torch.full(self.dims[a], fill) for k, a in self.sd_keys.items()} for _ in self.sets]

    def call(self, method, mappings, tau=0.005):
        f = getattr(self.obj, method)
        if method != "soft_update_from":
            return f(*mappings) if self.twin else f(mappings[0])
        return f(*mappings, tau=tau) if self.twin else f(mappings[0], tau)

    def untouched(self):
        """Every weight tensor is the same object with the same values and the staleness state is as `bare` left it."""
        return all(getattr(ws, a) is t and bool((t == 3.0).all()) and ws._packed == ("key", "stream") and ws.packs == 0
                   for ws, kept in zip(self.sets, self.kept) for a, t in kept.items()) and self.obj.packs == 0


def bad_tensors(shape):
    view = torch.ones(shape[::-1]).T
    assert tuple(view.shape) == tuple(shape) and not view.is_contiguous()
    return {"float64": torch.ones(shape, dtype=torch.float64), "view": view, "shape": torch.ones(shape[0], shape[1] - 1),
            "list": torch.ones(shape).tolist()}


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("cls,dims,n_nets", CASES)
def test_a_refused_mapping_changes_nothing_in_any_net(cls, dims, n_nets, method):
    s = Subject(cls, dims, n_nets)
    shape = dims[s.sd_keys[WIDE]]
    for net in range(n_nets):                                 # the bad mapping is net 1's, then net 2's alone
        for name, bad in bad_tensors(shape).items():
            m = s.mappings()
            m[net][WIDE] = bad
            if method == "load_state_dict" and name != "shape":
                continue                                      # converted, see test_load_state_dict_copies_and_converts
            with pytest.raises(ValueError):
                s.call(method, m)
            assert s.untouched(), (net, name)
        m = s.mappings()
        del m[net]["fc1.bias"]
        with pytest.raises(KeyError):
            s.call(method, m)
        # a missing key is named before any bad tensor, of every net (the blend checks net after net: of the same net)
        m[net if method == "soft_update_from" else 0][WIDE] = torch.ones(shape[::-1])
        with pytest.raises(KeyError):
            s.call(method, m)
        assert s.untouched(), net


@pytest.mark.parametrize("cls,dims,n_nets", CASES)
def test_load_state_dict_copies_and_converts(cls, dims, n_nets):
    s = Subject(cls, dims, n_nets)
    bad = bad_tensors(dims[s.sd_keys[WIDE]])
    for name in ("float64", "view", "list"):
        m = s.mappings(fill=2.0)
        m[-1][WIDE] = bad[name] * 5.0 if name != "list" else [[5.0] * len(r) for r in bad[name]]
        s.call("load_state_dict", m)
        for ws, kept in zip(s.sets, s.kept):                  # copied into the same tensors, float32
            assert all(getattr(ws, a) is t and t.dtype == torch.float32 for a, t in kept.items())
            assert ws._packed == ("key", "stream")            # copy_ advances the version counters: nothing else to mark
        assert float(getattr(s.sets[-1], s.sd_keys[WIDE]).min()) == 5.0 and float(s.sets[0].b1.max()) == 2.0
    got = s.obj.state_dict()
    assert [set(d) for d in (got if s.twin else [got])] == [set(s.sd_keys)] * n_nets


@pytest.mark.parametrize("cls,dims,n_nets", CASES)
def test_soft_update_from_refuses_and_changes_nothing(cls, dims, n_nets):
    s = Subject(cls, dims, n_nets)
    sd = s.mappings()
    for tau in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            s.call("soft_update_from", sd, tau)
    with pytest.raises(ValueError):
        s.call("soft_update_from", [object()] * n_nets)
    if s.twin:
        with pytest.raises(ValueError):                       # one mapping too many
            s.call("soft_update_from", sd + sd[:1])
    with pytest.raises(ValueError):                           # the target's own tensors
        s.call("soft_update_from", [{k: getattr(ws, a) for k, a in s.sd_keys.items()} for ws in s.sets])
    assert s.untouched()
    # CPU tensors: refused by a target that lives on a HIP device (ValueError: the tensor's device), and by a target that
    # itself claims the CPU (RuntimeError: there is no CPU form of the kernel)
    with pytest.raises(RuntimeError):
        s.call("soft_update_from", sd)
    assert s.untouched()
    s2 = Subject(cls, dims, n_nets, "cuda:0")
    with pytest.raises(ValueError):
        s2.call("soft_update_from", sd)
    assert s2.untouched()


@pytest.mark.parametrize("cls,dims,n_nets", CASES)
def test_share_state_dict_takes_tensors_by_reference(cls, dims, n_nets):
    s = Subject(cls, dims, n_nets)
    nets = [{k: torch.nn.Parameter(v) for k, v in m.items()} for m in s.mappings()]      # a learner's parameters
    s.call("share_state_dict", [{k: v.detach() for k, v in net.items()} for net in nets])  # what state_dict() returns
    for ws, net in zip(s.sets, nets):
        for k, a in s.sd_keys.items():
            assert getattr(ws, a).data_ptr() == net[k].data_ptr() and not getattr(ws, a).requires_grad
        assert ws._packed == ("key", "stream")                # the new tensors' keys differ: nothing else to mark
    ws, before = s.sets[-1], s.sets[-1].W2._version
    with torch.no_grad():
        nets[-1][WIDE].add_(1.0)                              # an optimiser step: in place, under no_grad
    assert ws.W2._version > before and float(ws.W2[0, 0]) == 2.0
    kept = [ws.W2 for ws in s.sets]
    for name, bad in bad_tensors(dims["W2"]).items():
        m = [{k: v.detach() for k, v in net.items()} for net in nets]
        m[-1][WIDE] = bad
        with pytest.raises(ValueError):
            s.call("share_state_dict", m)
        assert all(ws.W2 is t for ws, t in zip(s.sets, kept)), name   # a refused mapping changes nothing


@pytest.mark.parametrize("cls,dims,n_nets", CASES)
def test_the_stale_key_follows_the_packed_tensors_only(cls, dims, n_nets):
    s = Subject(cls, dims, n_nets)
    last = s.sets[-1]

    def current():                                            # what a rebuild leaves behind
        for ws in s.sets:
            if ws._stale() is not None:
                ws._packed = (ws._stale()[0], "stream")
        assert all(ws._stale() is None for ws in s.sets)
        return last._packed[0]

    def only_the_last_is_stale(key):
        assert all(ws._stale() is None for ws in s.sets[:-1])
        assert last._stale() is not None and last._stale()[0] != key
        assert [t.data_ptr() for t in last._stale()[1]] == [getattr(last, a).data_ptr() for a in last._PACKED]
    assert all(ws._stale() is not None for ws in s.sets)      # nothing was packed yet
    key = current()
    assert all(ws._stale() is None for ws in s.sets)          # asking changes nothing
    for a in last._PACKED:
        with torch.no_grad():
            getattr(last, a).add_(1.0)                        # updated in place
        only_the_last_is_stale(key)
        key = current()
        setattr(last, a, getattr(last, a).clone())            # replaced
        only_the_last_is_stale(key)
        key = current()
    assert "b2" in last._WEIGHTS and "b2" not in last._PACKED
    with torch.no_grad():
        last.b2.add_(1.0)
    last.b2 = last.b2.clone()
    assert all(ws._stale() is None for ws in s.sets)          # the kernel reads b2 as it is
    s.obj.mark_stale()
    assert all(ws._stale() is not None and ws._packed == (None, "stream") for ws in s.sets)
    assert last._stale()[0] == key                            # the tensors did not change: the mark is in the cache slot
    current()
    assert s.obj.packs == 0


def test_packed_names_are_weights():
    assert ACT.BatchedActor._PACKED == ("W1", "b1", "ln1_w", "ln1_b", "W2", "Wmu")
    for cls in (ACT.BatchedActor, CR.BatchedCritic, MC._Net):
        assert set(cls._PACKED) <= set(cls._WEIGHTS) == set(cls._SD.values())
    assert MC.BatchedTwinCritic._SD is MC._Net._SD
