"""NoveltyDetecter: the reference's train-and-test driver
(novelty_detection.py:10-127) without pytorch-ignite, on the native hot path.

train (:88-127): Adam(lr 1e-3) (:90); a trainer Engine running
``AutoEncoder.step`` per mini-batch and an evaluator Engine running
``AutoEncoder.validate`` over the valid loader at every EPOCH_COMPLETED
(:103-108); ``model.attach`` puts ignite-style RunningAverage(alpha 0.98,
reset per epoch) 'recon' metrics on both; the evaluator keeps a deep copy of
the state_dict whenever its EMA beats the lowest so far (:114-122); after
``n_epochs`` the best state is loaded back (:125).

test (:15-85): BASE (:42-47), SAP (:50-60) and NAP (:62-73) scores with
AUROC / AUPR / F1 / precision / recall.  The scores are produced on the
device: BASE and SAP from the fused scoring pass (mmad_ae_score_stream:
per-window squared-diff sums, the diffs never materialised), NAP from the
device diffs (mmad_ae_score) through the native NAP run; the metrics by the
native rank/threshold kernels (metric.py).  ``config.nap_fit_stream``: the
NAP fit is accumulated from the scoring pass over the train windows instead
(mmad_ae_nap_fit_stream; the train diffs are never materialised).  Train diffs are scored in batches
of ``config.batch_size`` and valid/test in 698 (:36-38, get_diffs' default).

Data parallel (model.dist set by dist.attach_data_parallel):
the loaders hand each rank its rows of every global batch, validation losses
are summed over the ranks (every rank keeps the same best-on-valid state),
BatchNorm running statistics are averaged over the ranks at every epoch end
before validation, and scoring is sharded by rows with the per-window scores
(and the NAP fit's train diffs) all-gathered, so every rank reports the
single-process metrics.
"""
from copy import deepcopy

import numpy as np
import torch

from . import metric
from .engine_loop import Engine, Events
from .reconstruction_aggregation import (NapScorer, base_from_layer_sq, sap_from_layer_sq,
                                         score_windows)


def _layer_sq(model, x, batch_size):
    return score_windows(x.to(model._native.device).float().contiguous(), model,
                         batch_size=batch_size, graph=False)


def _device_diffs(model, x, batch_size):
    """Concatenated get_diffs output [N, sum widths] on the device."""
    nat = model._native
    x = x.to(nat.device).float()
    parts = [nat.score(x[s:s + batch_size], want_diffs=True)[1] for s in range(0, x.shape[0], batch_size)]
    nat.check_status()
    return torch.cat(parts, dim=0)


def _stream_nap(model, x, batch_size, nap):
    """NAP scores [N] of x from the fused scoring pass (``nap`` attached to model)."""
    x = x.to(model._native.device).float().contiguous()
    _, scores = score_windows(x, model, batch_size=batch_size, graph=False, nap=nap)
    model._native.check_status()
    return scores


def _nap_model(model, cfg):
    """The model whose diffs NAP consumes.  NAP standardises every principal
    component of the train diffs by its variance (utils/normalize.py:36-45,
    utils/metric.py:219-222), down to ~1e-10 of the largest on these models,
    so bf16 activations -- 8 significant bits -- turn the low-variance
    components into quantisation noise: bf16 scoring of one fp32-trained
    model moved NAP AUROC by ~0.1 while BASE / SAP moved < 0.001
    (profiles/r03v_e2e_bf16_training.json).  For a bf16 model NAP therefore
    reads the diffs of an fp32 eval twin built from the same fp32 master
    weights and BN statistics (the reference's own precision); BASE / SAP stay
    on the bf16 path.  ``config.nap_dtype = 'model'`` keeps the model's own.
    The twin is built from a copy of the config, so it inherits
    ``config.score_dtype`` ('bf16x3': its diffs come from the split-bf16 GEMMs)."""
    if getattr(model, "mmad_dtype", "f32") == "f32" or getattr(cfg, "nap_dtype", "f32") != "f32":
        return model
    import types
    from .model_builder import get_model
    tcfg = types.SimpleNamespace(**vars(cfg))
    tcfg.dtype = "f32"
    tcfg.gpu_id = model._native.device.index
    twin = get_model(tcfg)
    twin.load_state_dict(model.state_dict())
    twin.eval()
    return twin


class NoveltyDetecter:
    def __init__(self, config):
        self.config = config

    # ------------------------------------------------------------------ test
    def scores(self, model, train_x, valid_x, test_x):
        """(valid, test) score pairs per method: {'base','sap','nap'} ->
        (valid_score [Nv], test_score [Nt]) fp32 device tensors."""
        cfg = self.config
        model.eval()
        nat = model._native
        widths = nat.diff_widths()
        n = len(widths)
        start = getattr(cfg, "start_layer_index", 0)
        end = cfg.n_layers + 1 - getattr(cfg, "end_layer_index", -1)   # novelty_detection.py:57
        dp = model.dist if getattr(model, "dist", None) is not None and model.dist.world > 1 else None
        fit_stream = bool(getattr(cfg, "nap_fit_stream", False))
        if fit_stream and getattr(cfg, "train_diffs", None):
            raise ValueError("config.nap_fit_stream never materialises the train diffs that "
                             "config.train_diffs would save")
        if fit_stream and dp is not None:
            raise ValueError("config.nap_fit_stream is single-process: a data-parallel fit would "
                             "all-reduce its sums, which is not implemented")

        def rows(fn, x):
            # per-window rows of fn(x): this rank's shard, all-gathered (DP)
            if dp is None:
                return fn(x)
            return dp.gather(fn(dp.shard(x)), x.shape[0])

        out = {}
        with torch.no_grad():
            # [n_layers+1, N] per-layer sums, gathered along the windows
            lv = rows(lambda v: _layer_sq(model, v, 698).t().contiguous(), valid_x).t()
            lt = rows(lambda v: _layer_sq(model, v, 698).t().contiguous(), test_x).t()
            out["base"] = (base_from_layer_sq(lv, widths), base_from_layer_sq(lt, widths))
            out["sap"] = (sap_from_layer_sq(lv, widths, start, end), sap_from_layer_sq(lt, widths, start, end))
            nap = NapScorer(model, start_layer_index=start, end_layer_index=end)
            cuts = np.cumsum([0] + widths)
            nap_sel = nap.sel
            sel = slice(int(cuts[nap_sel.start]), int(cuts[min(nap_sel.stop, n)]))
            nm = _nap_model(model, cfg)
            if fit_stream:
                # opt-in: the fit accumulated from the scoring pass over the train
                # windows, batch by batch (the train diffs are never materialised)
                nap = NapScorer.standalone(sel.stop - sel.start, device=nat.device).fit_stream(
                    nm, train_x, cfg.batch_size, layers=(nap_sel.start, min(nap_sel.stop, n)))
            else:
                nap_train = rows(lambda v: _device_diffs(nm, v, cfg.batch_size)[:, sel].contiguous(), train_x)
                path = getattr(cfg, "train_diffs", None)
                if path and (dp is None or torch.distributed.get_rank(dp.group) == 0):
                    torch.save(nap_train.cpu(), path)           # utils/metric.py:205
                nap = NapScorer.standalone(nap_train.shape[1], device=nat.device).fit(train_diffs=nap_train)
                del nap_train
            if getattr(cfg, "nap_stream", False):
                # opt-in: valid / test NAP from the fused scoring pass (the diffs
                # stay in the workspace); config.nap_precision picks the NAP GEMM
                nap.attach(nm, precision=getattr(cfg, "nap_precision", "f32"),
                           layers=(nap_sel.start, min(nap_sel.stop, n)))
                out["nap"] = (rows(lambda v: _stream_nap(nm, v, 698, nap), valid_x),
                              rows(lambda v: _stream_nap(nm, v, 698, nap), test_x))
                nap.detach()
            else:
                out["nap"] = (rows(lambda v: nap.score(_device_diffs(nm, v, 698)[:, sel]), valid_x),
                              rows(lambda v: nap.score(_device_diffs(nm, v, 698)[:, sel]), test_x))
            del nm
        return out

    def online_scorer(self, model, train_x, valid_x, rows=None):
        """The deployment form of ``scores``: an online.OnlineScorer over
        ``model`` that returns BASE, SAP and NAP of up to ``rows`` (16 or 64)
        windows per call from one replayed graph.  rows=None: 16, or 64 when
        ``config.slicing_size`` (the deployment loop's window count) is
        17..64.  NAP is fitted on ``train_x`` as ``scores``
        fits it (``config.nap_fit_stream`` honoured); for a bf16 model the
        whole online path runs on the fp32 twin of ``_nap_model`` (NAP needs
        fp32 diffs and one graph is to produce all three scores).  The
        thresholds are calibrated on ``valid_x`` (metric.threshold_metrics'
        quantile rule on the batch route's validation scores).
        ``config.online_groups`` (absent: off) on a model whose input is the
        fused HSR row: the scorer also returns the per-modality scores of
        hsr_net.modality_columns(), their thresholds calibrated on the batch
        route's group scores of ``valid_x`` by the same rule.  Single
        process."""
        from .hsr_net import FUSED_WIDTH, modality_columns
        from .online import OnlineScorer, rows_for
        from .reconstruction_aggregation import group_scores
        cfg = self.config
        model.eval()
        start = getattr(cfg, "start_layer_index", 0)
        end = cfg.n_layers + 1 - getattr(cfg, "end_layer_index", -1)
        if rows is None:
            rows = rows_for(getattr(cfg, "slicing_size", None))
        with torch.no_grad():
            nm = _nap_model(model, cfg)
            nat = nm._native
            widths = nat.diff_widths()
            n = len(widths)
            nap = NapScorer(nm, start_layer_index=start, end_layer_index=end)
            layers = (nap.sel.start, min(nap.sel.stop, n))
            cuts = np.cumsum([0] + widths)
            sel = slice(int(cuts[layers[0]]), int(cuts[layers[1]]))
            if bool(getattr(cfg, "nap_fit_stream", False)):
                nap.fit_stream(nm, train_x, cfg.batch_size, layers=layers)
            else:
                nap.fit(train_diffs=_device_diffs(nm, train_x, cfg.batch_size)[:, sel].contiguous())
            # (the layout scores() reduces: the same validation scores to the bit)
            lv = _layer_sq(nm, valid_x, 698).t().contiguous().t()
            valid = {"base": base_from_layer_sq(lv, widths), "sap": sap_from_layer_sq(lv, widths, start, end),
                     "nap": nap.score(_device_diffs(nm, valid_x, 698)[:, sel])}
            groups = None
            if bool(getattr(cfg, "online_groups", False)) and widths[0] == FUSED_WIDTH:
                groups = modality_columns()
            scorer = OnlineScorer(nm, nap=nap, start_layer_index=start, end_layer_index=end, rows=rows,
                                  groups=groups)
            if groups is not None:
                gs = group_scores(torch.as_tensor(valid_x), nm, scorer.groups)
                valid["groups"] = dict(zip(scorer.group_names, gs))
            scorer.calibrate(valid)
        return scorer

    def online_bank(self, models, train_x, valid_x, rows=None):
        """The fused detector and its unimodal siblings as one
        online.SensorBank: ``models`` maps config.sensor names ('All',
        'hand_camera', 'head_depth', 'force_torque', 'mic') to trained models
        (one per ``--sensor`` setting, 1..8 of them; each of this detecter's
        ``config`` layer settings).  Every member's scorer is built by
        ``online_scorer`` on that sensor's columns of the fused rows
        ``train_x`` / ``valid_x`` [N, 1728] -- its own NAP fit and calibrated
        thresholds -- and the bank scores them all from one shared row per
        tick, sharing launches (DESIGN.md §4 "Sensor bank").  The bank shares
        one fused HSR_Net: the unimodal models are expected to have been
        trained on that network's blocks of the fused row."""
        from .hsr_net import FUSED_WIDTH, modality_columns
        from .online import SENSOR_KEYS, SensorBank
        cols = modality_columns()
        scorers, starts = {}, {}
        for name, model in models.items():
            if name not in SENSOR_KEYS:
                raise ValueError(f"online_bank: unknown sensor {name!r} ({', '.join(SENSOR_KEYS)})")
            c0, c1 = (0, FUSED_WIDTH) if SENSOR_KEYS[name] is None else cols[SENSOR_KEYS[name]]
            tx, vx = (torch.as_tensor(v).reshape(len(v), -1)[:, c0:c1].contiguous() for v in (train_x, valid_x))
            scorers[name] = self.online_scorer(model, tx, vx, rows=rows)
            starts[name] = c0
        return SensorBank(scorers, starts, width=FUSED_WIDTH)

    def test(self, model, dset_manager, train_loader, valid_loader, test_loader, df_test=None):
        """novelty_detection.py:15-85.  Returns ((base_auroc, base_aupr),
        (sap_auroc, sap_aupr), (nap_auroc, nap_aupr), df_test) with df_test a
        list of result rows (the reference appends to a pandas DataFrame)."""
        cfg = self.config
        model.eval()
        with torch.no_grad():
            train_x, _ = dset_manager.get_transformed_data(train_loader)
            valid_x, _ = dset_manager.get_transformed_data(valid_loader)
            test_x, test_y = dset_manager.get_transformed_data(test_loader)
        test_y = np.asarray(test_y)
        if getattr(cfg, "unimodal_normal", False):
            test_y = np.where(np.isin(test_y, [cfg.target_class]), False, True)
        else:
            test_y = np.where(np.isin(test_y, [cfg.target_class]), True, False)
        self.model = model
        self.last_inputs = (train_x, valid_x, test_x, test_y)
        sc = self.scores(model, train_x, valid_x, test_x)
        row = {}
        res = {}
        for name in ("base", "sap", "nap"):
            v, t = sc[name]
            auroc, aupr, _, _ = metric.rank_metrics(t, test_y)
            thr = metric.threshold_metrics(v, t, test_y)
            row.update({f"{name}_auroc": auroc, f"{name}_aupr": aupr, f"{name}_f1score": thr[1],
                        f"{name}_precision": thr[4], f"{name}_recalls": thr[5]})
            res[name] = (auroc, aupr)
        self.last_scores = {k: (v.cpu().numpy(), t.cpu().numpy()) for k, (v, t) in sc.items()}
        self.last_row = row
        self.last_test_label = test_y
        df_test = list(df_test or []) + [row]
        return res["base"], res["sap"], res["nap"], df_test

    # ----------------------------------------------------------------- train
    def train(self, model, train_loader, valid_loader):
        """novelty_detection.py:88-127."""
        optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
        trainer = Engine(model.step)
        trainer.model, trainer.optimizer, trainer.config = model, optimizer, self.config
        trainer.train_history = []
        trainer.test_history = []
        evaluator = Engine(model.validate)
        evaluator.model, evaluator.config, evaluator.lowest_loss = model, self.config, np.inf
        evaluator.valid_history = []
        evaluator.best_model = None
        evaluator.best_epoch = 0
        model.attach(trainer, evaluator, self.config)

        def run_validation(engine, evaluator, valid_loader):
            evaluator.run(valid_loader, max_epochs=1)

        if getattr(model, "dist", None) is not None:
            # data parallel: per-shard BN running statistics averaged for eval
            # (and the sharded master weights gathered before any state_dict copy)
            trainer.add_event_handler(Events.EPOCH_COMPLETED,
                                      lambda engine: model.dist.epoch_end(model))
        trainer.add_event_handler(Events.EPOCH_COMPLETED, run_validation, evaluator, valid_loader)
        # every mini-batch's loss (the reference's step output), for trajectory checks
        self.step_losses = []
        trainer.add_event_handler(Events.ITERATION_COMPLETED,
                                  lambda engine: self.step_losses.append(float(engine.state.output[0])))

        @trainer.on(Events.EPOCH_COMPLETED)
        def append_train_loss_history(engine):
            engine.train_history += [float(engine.state.metrics["recon"])]

        @evaluator.on(Events.EPOCH_COMPLETED)
        def append_valid_loss_history(engine):
            loss = float(engine.state.metrics["recon"])
            if loss < engine.lowest_loss:
                engine.lowest_loss = loss
                engine.best_model = deepcopy(engine.model.state_dict())
                engine.best_epoch = trainer.state.epoch
            engine.valid_history += [loss]

        trainer.run(train_loader, max_epochs=self.config.n_epochs)
        if evaluator.best_model is not None:
            model.load_state_dict(evaluator.best_model)
        self.best_epoch = evaluator.best_epoch
        return trainer.train_history, evaluator.valid_history, trainer.test_history, model


def main(config):
    """novelty_detection.py:177-211 on the synthetic dataset (one process per
    GPU under torchrun: data parallel, dist.attach_data_parallel)."""
    from . import dist as mdist
    from .data_loaders import get_input_size, get_loaders
    from .model_builder import get_model
    if getattr(config, "input_size", None) is None:
        config.input_size = get_input_size(config)
    rank, world, _ = mdist.init_from_env()
    model = get_model(config)
    if world > 1:
        mdist.attach_data_parallel(model)
    detecter = NoveltyDetecter(config)
    dset_manager, train_loader, valid_loader, test_loader = get_loaders(config, rank=rank, world=world)
    _, _, _, model = detecter.train(model, train_loader, valid_loader)
    if getattr(config, "saved_name", None) and rank == 0:
        torch.save(model.state_dict(), config.saved_name)
    return detecter.test(model, dset_manager, train_loader, valid_loader, test_loader)[:3]
