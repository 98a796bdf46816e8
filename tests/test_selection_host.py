"""lpformer_amd/selection.py without a GPU: the three workspace forms on CPU tensors, driven by fake launches that write
the control block, ``blk_cnt`` and the totals per type the way the kernels do (counting what a batch needs even where
the buffers are too small, raising the sticky bits then).  The model's side -- look up the workspace, size it if needed,
launch -- runs through ``LinkTransformer``'s own methods on a stand-in object.

Every expected size is written out from the formulas the code had before this module existed (link_transformer.py's
three workspace classes and three first-batch sizings), not computed with the module's functions."""
import contextlib
import types

import pytest
import torch

from lpformer_amd import _lib, selection
from lpformer_amd import link_transformer as LT

SIZES = (1, 64, 65, 700)
NBLK = {1: 1, 64: 1, 65: 2, 700: 11}           # blocks of 64 pairs
CPU = torch.device("cpu")
NODE_RANGE, ITEM_CAP, ENTRY_CAP = 1, 2, 4      # (pinned against the header by tests/test_abi_bindings_host.py)


class Host:
    """Stand-in for the model: LinkTransformer's selection methods over fake launches.  ``counts``: what the fake
    kernels report about every batch -- need / slots / kept (lpf_select4), items / tot (plan + run, regions)."""

    _sel_ws = LT.LinkTransformer._sel_ws
    _select_device = LT.LinkTransformer._select_device
    _select_regions_device = LT.LinkTransformer._select_regions_device
    _select4_device = LT.LinkTransformer._select4_device
    check_selection = LT.LinkTransformer.check_selection

    def __init__(self, monkeypatch, regions=True, **counts):
        self._ws, self.device, self.num_nodes, self.regions = {}, CPU, 1000, regions
        self.counts = dict(dict(need=5000, slots=4000, kept=[300, 0, 45], items=100, tot=[700, 9000, 20], bits=0), **counts)
        self.log, self.raw, self.on_stream = [], 7, []
        monkeypatch.setattr(LT, "raw_stream", lambda dev: self.raw)

        @contextlib.contextmanager
        def on(stream):                      # (torch.cuda.stream: which stream the status was read / cleared under)
            self.on_stream.append(stream)
            yield
        monkeypatch.setattr(torch.cuda, "stream", on)

    def _uses_select4_regions(self, adj_mask=None):
        return self.regions and adj_mask is None

    def _select_graphs(self, test_set, adj_mask=None):
        return "graphs"

    def _select4_shape(self, bs, slots):
        self.shape_args = (bs, slots)
        return 512

    def _select_launch(self, ws, batch, graphs):
        c = self.counts
        self.log.append("plan_run")
        ws.ctl[0], ws.ctl[1] = 16 * batch.shape[1], c["items"]
        ws.ctl[4:7] = torch.tensor(c["tot"])
        ws.ctl[3] |= c["bits"] | (ITEM_CAP if c["items"] > ws.item_cap else 0) | \
            (ENTRY_CAP if max(c["tot"]) > ws.ent_cap else 0)

    def _select4_launch(self, ws, batch, wi, q=None):
        c = self.counts
        self.log.append("select4" if q is None else "select4_q")
        entries, cap = ws.pair_major
        assert cap == 0 or entries.numel() == 4 * cap
        ws.ctl[0], ws.ctl[1] = c["need"], c["slots"]
        fits = c["need"] <= cap
        ws.blk_cnt.zero_()
        if fits:
            kept = c["kept"][:NBLK[batch.shape[1]]]
            ws.blk_cnt[0:2 * len(kept):2] = torch.tensor(kept, dtype=torch.int32)
        ws.ctl[3] |= c["bits"] | (0 if fits else ENTRY_CAP)

    def _regions_launch(self, ws, batch, wi):
        self._select4_launch(ws, batch, wi)
        self.log.append("regions")
        ws.ctl[4:7] = torch.tensor(self.counts["tot"])
        ws.ctl[3] |= ENTRY_CAP if max(self.counts["tot"]) > ws.ent_cap else 0

    def took(self):
        out, self.log = self.log, []
        return out


def _batch(bs):
    return torch.zeros(2, bs, dtype=torch.int64)


def _numel(ws):
    return {k: (v.numel(), v.dtype) for k, v in vars(ws).items() if isinstance(v, torch.Tensor)}


@pytest.mark.parametrize("bs", SIZES)
def test_fixed_buffers_of_the_three_forms(bs):
    i32, i64 = torch.int32, torch.int64
    plan_lb = int(_lib.hip().lpf_select_plan_blocks(bs)) + 1
    assert _numel(selection.PlanRunWorkspace(CPU, bs)) == {
        "ctl": (16, i64), "desc": (16 * bs, i64), "offs": (bs + 1, i64), "plan_lb": (plan_lb, i64),
        "type_ptr": (3 * (bs + 1), i32)}
    assert _numel(selection.PairMajorWorkspace(CPU, bs)) == {
        "ctl": (32, i64), "pair_tab": (4 * bs, i32), "blk_cnt": (2 * NBLK[bs] + 2, i32)}
    assert _numel(selection.RegionsWorkspace(CPU, bs)) == {
        "ctl": (32, i64), "pair_tab": (4 * bs, i32), "blk_cnt": (2 * NBLK[bs] + 2, i32),
        "blk_types": (4 * NBLK[bs] + 4, i32), "type_ptr": (3 * (bs + 1), i32)}
    for cls in (selection.PlanRunWorkspace, selection.PairMajorWorkspace, selection.RegionsWorkspace):
        ws = cls(CPU, bs)
        assert not ws.calibrated and not ws.ctl.any() and ws.ent_cap == 0 and ws.entries is None
    assert not hasattr(selection.PairMajorWorkspace(CPU, bs), "blk_types")     # (how bench.py tells the forms apart)
    for name in ("item_pair", "run_lb", "item_cap", "kept_cap"):               # (fields of the other forms)
        assert not hasattr(selection.RegionsWorkspace(CPU, bs), name)


def test_sizing_formulas():
    assert selection.TOKEN == 16
    assert [selection.first_item_room(bs) for bs in SIZES + (5000,)] == [4112, 4112, 4112, 4112, 5016]
    assert selection.item_room(10000) == 2 * 10000 + 16
    assert selection.region_room([700, 9000, 20]) == 2 * 9000 + 4096
    assert selection.slot_room(5000) == 3 * 5000 + 65536
    assert selection.kept_room(345) == 2 * 345 + 65536
    assert [selection.blocks(bs) for bs in SIZES] == [NBLK[bs] for bs in SIZES]
    assert (selection.CTL_ROOM, selection.CTL_ITEMS, selection.CTL_ERR, selection.CTL_TOTALS) == (0, 1, 3, slice(4, 7))


@pytest.mark.parametrize("bs", SIZES)
def test_pair_major_first_batch_and_later_batches(monkeypatch, bs):
    m = Host(monkeypatch)
    ws = m._select4_device(_batch(bs), False)
    assert m.took() == ["select4", "select4", "select4"]            # token buffer, sized buffer, the batch itself
    kept = sum(m.counts["kept"][:NBLK[bs]])
    assert ws is m._ws[("sel4", 7, bs)] and ws.calibrated and int(ws.ctl[3]) == 0
    assert (ws.ent_cap, ws.entries.numel(), ws.kept_cap) == (3 * 5000 + 65536, 4 * (3 * 5000 + 65536), 2 * kept + 65536)
    assert m.shape_args == (bs, 4000) and ws.shape == 512
    assert m._select4_device(_batch(bs), False, q=("y", "out")) is ws
    assert m.took() == ["select4_q"]                                # (a sized workspace: the launch and nothing else)
    assert m.on_stream == [None, None]                              # ONE status read + its clear, on the current stream


@pytest.mark.parametrize("bs", SIZES)
def test_regions_first_batch_and_later_batches(monkeypatch, bs):
    m = Host(monkeypatch)
    ws = m._select_device(_batch(bs), False)
    assert m.took() == ["select4", "select4", "regions", "select4", "regions"]
    assert isinstance(ws, selection.RegionsWorkspace) and ws is m._ws[("sel2", 7, bs)]
    assert ws.calibrated and int(ws.ctl[3]) == 0
    assert (ws.ent_cap4, ws.entries4.numel()) == (3 * 5000 + 65536, 4 * (3 * 5000 + 65536))
    assert (ws.ent_cap, ws.entries.numel()) == (2 * 9000 + 4096, 3 * 4 * (2 * 9000 + 4096))
    assert m.shape_args == (bs, 4000) and ws.shape == 512
    assert m._select_device(_batch(bs), False) is ws and m.took() == ["select4", "regions"]
    # the other form under the same key replaces it, and the other way round
    m.regions = False
    other = m._select_device(_batch(bs), False)
    assert isinstance(other, selection.PlanRunWorkspace) and m._ws[("sel2", 7, bs)] is other and m._sel_ws(7, bs) is other
    m.regions = True
    assert isinstance(m._select_device(_batch(bs), False), selection.RegionsWorkspace)


@pytest.mark.parametrize("bs", SIZES)
@pytest.mark.parametrize("items, launches", [(100, 1), (10000, 2)])
def test_plan_run_first_batch_and_later_batches(monkeypatch, bs, items, launches):
    m = Host(monkeypatch, regions=False, items=items)
    ws = m._select_device(_batch(bs), False)
    assert m.took() == ["plan_run"] * (launches + 1)                # (a plan of more items than 4,112 is made again)
    assert isinstance(ws, selection.PlanRunWorkspace) and ws.calibrated and int(ws.ctl[3]) == 0
    item_cap = max(4096 + 16, 2 * items + 16)                       # (work items are never given back)
    assert (ws.item_cap, ws.item_pair.numel()) == (item_cap, item_cap)
    assert ws.run_lb.numel() * ws.run_lb.element_size() == 3 * 8 * item_cap and not ws.run_lb.any()
    assert (ws.ent_cap, ws.entries.numel()) == (2 * 9000 + 4096, 3 * 4 * (2 * 9000 + 4096))
    assert m._select_device(_batch(bs), False, None) is ws and m.took() == ["plan_run"]


def test_item_cap_that_stays_raises_after_three_attempts(monkeypatch):
    m = Host(monkeypatch, regions=False, bits=ITEM_CAP)
    with pytest.raises(_lib.LpfError, match="could not be sized"):
        m._select_device(_batch(65), False)
    assert m.took() == ["plan_run"] * 3
    ws = m._ws[("sel2", 7, 65)]
    assert not ws.calibrated and int(ws.ctl[3]) == 0


@pytest.mark.parametrize("form", ["plan_run", "pair_major", "regions"])
def test_node_id_out_of_range_raises_and_leaves_the_status_cleared(monkeypatch, form):
    m = Host(monkeypatch, regions=form == "regions", bits=NODE_RANGE)
    select = m._select4_device if form == "pair_major" else m._select_device
    with pytest.raises(IndexError, match=r"batch holds node ids outside \[0, 1000\)"):
        select(_batch(65), False)
    assert len(m.took()) == 1                                       # (the first token launch; nothing after it)
    (ws,) = m._ws.values()
    assert int(ws.ctl[3]) == 0 and not ws.calibrated
    # ... and from the synchronising check of a sized workspace
    m.counts["bits"] = 0
    ws = select(_batch(65), False)
    ws.ctl[3] = NODE_RANGE | ENTRY_CAP
    with pytest.raises(IndexError, match="batch holds node ids outside"):
        m.check_selection(types.SimpleNamespace(cuda_stream=7))
    assert int(ws.ctl[3]) == 0


def test_growth_rule():
    assert selection.needs_resize(0, 16, False) and selection.needs_resize(100, 101, False)
    assert not selection.needs_resize(100, 100, False) and not selection.needs_resize(100, 3, False)
    assert selection.needs_resize(150, 74, True) and not selection.needs_resize(150, 75, True)     # below HALF only
    ws = selection.PairMajorWorkspace(CPU, 65)
    ws.ensure(ent_cap=100)
    first = ws.entries
    assert (ws.ent_cap, first.numel()) == (100, 400)
    ws.ensure(ent_cap=50)
    ws.ensure(ent_cap=50, shrink=True)                              # (not below half: 50 == 100 // 2)
    assert ws.entries is first and ws.ent_cap == 100
    ws.ensure(ent_cap=150)
    assert (ws.ent_cap, ws.entries.numel()) == (150, 600) and ws.entries is not first
    ws.ensure(ent_cap=8, shrink=True)                               # (what the GPU tests do to force an overflow)
    assert (ws.ent_cap, ws.entries.numel()) == (8, 32)
    for cls, words in ((selection.PlanRunWorkspace, 12), (selection.RegionsWorkspace, 12)):
        ws = cls(CPU, 65)
        ws.ensure(ent_cap=1000)
        ws.ensure(ent_cap=8, shrink=True)
        assert (ws.ent_cap, ws.entries.numel()) == (8, 8 * words)
    ws = selection.RegionsWorkspace(CPU, 65)
    assert ws._fit("entries4", 1000, 4) == 1000 and ws._fit("entries4", 500, 4, shrink=True) == 1000
    assert ws._fit("entries4", 499, 4, shrink=True) == 499 and (ws.entries4.numel(), ws.entries) == (4 * 499, None)
    ws = selection.PlanRunWorkspace(CPU, 65)
    ws.ensure(item_cap=1000, ent_cap=16)
    ws.ensure(item_cap=10, ent_cap=16, shrink=True)
    assert (ws.item_cap, ws.item_pair.numel(), ws.ent_cap) == (1000, 1000, 16)


def test_stream_check_sizes_again_after_an_overflow_and_looks_at_its_own_stream_only(monkeypatch):
    m = Host(monkeypatch)
    s7, s8 = types.SimpleNamespace(cuda_stream=7), types.SimpleNamespace(cuda_stream=8)
    mine = [m._select4_device(_batch(65), False), m._select_device(_batch(65), False)]
    m.raw = 8
    other = m._select4_device(_batch(65), False)
    m._ws[("att_rows", 7)] = torch.zeros(4)                         # (named scratch shares the dict)
    m.took()
    del m.on_stream[:]
    assert m.check_selection(s7) and m.on_stream == [s7, s7]        # (two reads, both under the stream asked for)
    for ws in mine + [other]:
        ws.ctl[3] = ENTRY_CAP
    del m.on_stream[:]
    assert m.check_selection(s7) is False
    assert m.on_stream == [s7] * 4                                  # (read + clear per workspace, under that stream)
    assert all(int(ws.ctl[3]) == 0 and not ws.calibrated for ws in mine)
    assert int(other.ctl[3]) == ENTRY_CAP and other.calibrated      # (another stream's: not looked at)
    assert m.check_selection(s7) is True
    m.raw = 7
    assert m._select4_device(_batch(65), False) is mine[0] and mine[0].calibrated    # sized again by the next batch
    assert m.took() == ["select4"] * 3
    assert m.check_selection(s8) is False and m.check_selection(s8) is True and not other.calibrated


def test_buffers_lists_every_tensor_of_each_form(monkeypatch):
    want = {"plan_run": ["ctl", "desc", "offs", "plan_lb", "type_ptr", "item_pair", "run_lb", "entries"],
            "pair_major": ["ctl", "pair_tab", "blk_cnt", "entries"],
            "regions": ["ctl", "pair_tab", "blk_cnt", "blk_types", "type_ptr", "entries", "entries4"]}
    for form, names in want.items():
        m = Host(monkeypatch, regions=form == "regions")
        ws = (m._select4_device if form == "pair_major" else m._select_device)(_batch(65), False)
        assert sorted(k for k, v in vars(ws).items() if isinstance(v, torch.Tensor)) == sorted(names)
        assert sorted(map(id, ws.buffers())) == sorted(id(getattr(ws, k)) for k in names)
        old = ws.entries
        ws.ensure(ent_cap=8, shrink=True)                           # a re-sized buffer is a new tensor: listed, the old one not
        assert any(b is ws.entries for b in ws.buffers()) and not any(b is old for b in ws.buffers())
