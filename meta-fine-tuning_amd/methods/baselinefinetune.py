"""BaselineFinetune: frozen features + a freshly trained head (mirror of methods/baselinefinetune.py:9-61): a linear head
(``loss_type='softmax'``, Baseline) or the cosine head backbone.distLinear (``loss_type='dist'``, Baseline++)."""
import numpy as np

from .. import backbone
from .meta_template import MetaTemplate, dist_head_adapt


class BaselineFinetune(MetaTemplate):
    def __init__(self, model_func, n_way, n_support, loss_type="softmax"):
        super().__init__(model_func, n_way, n_support)
        if loss_type not in ("softmax", "dist"):
            raise ValueError("loss_type must be 'softmax' or 'dist', got %r" % (loss_type,))
        self.loss_type = loss_type

    def set_forward(self, x, is_feature=True):
        return self.set_forward_adaptation(x, is_feature)       # Baseline always adapts

    def set_forward_adaptation(self, x, is_feature=True):
        if self.loss_type == "softmax":
            return super().set_forward_adaptation(x, is_feature)
        assert is_feature == True, 'Baseline only support testing with feature'  # noqa: E712
        z_support, z_query = self.parse_feature(x, is_feature)
        z_support = z_support.contiguous().view(1, self.n_way * self.n_support, -1).float()
        z_query = z_query.contiguous().view(1, self.n_way * self.n_query, -1).float()
        y_support = np.repeat(range(self.n_way), self.n_support)
        clf = backbone.distLinear(self.feat_dim, self.n_way)      # same torch-RNG draw as the torch weight-norm head
        # 100 permutations, then the 100 x ceil(S / 4) SGD steps in one launch and the query scores in another
        scores, _, _ = dist_head_adapt(z_support, y_support, z_query, clf.L.weight_v.data.unsqueeze(0),
                                       clf.L.weight_g.data.view(1, -1), self.n_way, self.n_support)
        return scores

    def set_forward_loss(self, x):
        raise ValueError('Baseline predict on pretrained feature and do not support finetune backbone')
