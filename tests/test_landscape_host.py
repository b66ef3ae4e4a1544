"""Host logic of the evaluation entry points: Config defaults of the reference, the CSV file names, weight-row validation and the
eigenvalue-bound split of the landscape (no GPU)."""
import pytest
import torch


def test_config_eval_defaults():
    from depth_correction_amd.config import Config, Loss
    cfg = Config()
    assert cfg.test_poses_path == [] and cfg.train_poses_path == [] and cfg.val_poses_path == []
    assert cfg.loss_eval_csv is None
    assert cfg.eval_losses == ['min_eigval_loss', 'trace_loss', 'icp_loss'] == list(Loss)
    back = Config().from_yaml(_yaml_tmp(Config(loss_eval_csv='x.csv')))
    assert back.loss_eval_csv == 'x.csv'


def _yaml_tmp(cfg):
    import tempfile
    import os
    path = os.path.join(tempfile.mkdtemp(), 'cfg.yaml')
    cfg.to_yaml(path)
    return path


def test_loss_eval_csv_names():
    from depth_correction_amd.config import loss_eval_csv
    assert loss_eval_csv('/log', 'trace_loss', 'test') == '/log/loss_eval_trace_loss_test.csv'
    assert loss_eval_csv('/log', 'icp_loss') == '/log/loss_eval_icp_loss.csv'
    assert loss_eval_csv('', 'min_eigval_loss', 'val') == 'loss_eval_min_eigval_loss_val.csv'


def test_weight_rows_shapes():
    from depth_correction_amd.eval import _weight_rows
    w = _weight_rows([0.0, 1.0, 2.0], 1, 'cpu')
    assert w.shape == (3, 1) and w.dtype == torch.float64
    assert _weight_rows(torch.zeros((5, 2)), 2, 'cpu').shape == (5, 2)
    with pytest.raises(ValueError):
        _weight_rows([0.0, 1.0], 2, 'cpu')
    with pytest.raises(ValueError):
        _weight_rows(torch.zeros((4, 3)), 2, 'cpu')
    with pytest.raises(ValueError):
        _weight_rows(torch.zeros((4, 1)), 0, 'cpu')


def test_model_with_weights_copies():
    from depth_correction_amd.eval import _model_with_weights
    from depth_correction_amd.model import Linear, ScaledPolynomial
    m = ScaledPolynomial(w=[0.0, 0.0], exponent=[2.0, 4.0])
    c = _model_with_weights(m, torch.tensor([1e-3, -2e-3], dtype=torch.float64))
    assert torch.equal(c.w.detach().reshape(-1), torch.tensor([1e-3, -2e-3], dtype=c.w.dtype))
    assert (m.w.detach() == 0).all()
    lin = _model_with_weights(Linear(), torch.tensor([0.9, 0.1, 0.2], dtype=torch.float64))
    assert [lin.w0.item(), lin.w1.item(), lin.b.item()] == pytest.approx([0.9, 0.1, 0.2])


def test_eig_bounds_split():
    from depth_correction_amd.config import Config
    from depth_correction_amd.eval import _eig_bounds
    cfg = Config(eigenvalue_bounds=[[0, None, 0.01]], eigenvalue_ratio_bounds=[[0, 1, 0, 0.25], [1, 2, 0.25, 1.0]])
    assert _eig_bounds(cfg) == [(0, -1, float('-inf'), 0.01), (0, 1, 0.0, 0.25), (1, 2, 0.25, 1.0)]
    assert _eig_bounds(Config(eigenvalue_ratio_bounds=[])) == []
