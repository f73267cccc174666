"""MI355X drop-in for ``mlp`` (`embedder_eDOS/mlp.py:11-35`): ``forward(g) -> dos [B, 201]``.

``Graphnetwork`` without message passing: node encoder, global encoder, decoder on cat[u, sum-pooled nodes], the output head
on cat[energy embedding, graph].  Parameter names and creation order are ``Graphnetwork``'s minus ``stacked_processor``;
``layers`` is ignored, as upstream.  ``GN_encoder.edge_encoder.*`` is computed and dropped upstream (`:27`): it is dead here
(``grad is None``, skipped by AdamW), like the node encoder the input width does not select.
(`mlp2` crashes upstream - `:51` calls the Encoder without its ``energies`` argument, `:76` - and so do `mlp_phonon` and
`mlp2_phonon` of `embedder_phDOS/mlp_phonon.py`, on the same Encoder arity: none of the three is provided.)"""
from torch import nn

from .. import functional as Fn
from .._blocks import Decoder, Encoder
from .._models import GraphnetworkBase

_EDGE_ENCODER = tuple(f"GN_encoder.edge_encoder.{s}" for s in ("0.weight", "0.bias", "1.weight", "2.weight", "2.bias"))


class mlp(GraphnetworkBase):
    _returns_x = False
    _has_f64_program = False
    _fwd_fn = staticmethod(Fn.mlp_fwd)

    @staticmethod
    def _bwd_fn(P, G, cfg, m, saved, ddos, dx, sink, factored_head=False):
        Fn.mlp_bwd(P, G, cfg, m, saved, ddos, sink, factored_head=factored_head)

    def __init__(self, layers, n_atom_feats, n_bond_feats, n_glob_feats, n_hidden, dim_out, device):
        super().__init__()
        self.embeddings = nn.Embedding(201, n_hidden)
        self.GN_encoder = Encoder(n_atom_feats, n_bond_feats, n_hidden, n_global_feats=n_glob_feats, prompt_branch=True)
        self.GN_decoder = Decoder(n_hidden * 2, n_hidden)
        self.device = device
        self.out_layer = nn.Sequential(nn.Linear(n_hidden * 2, n_hidden), nn.LeakyReLU(), nn.Linear(n_hidden, 1))
        self._cfg = Fn.ModelCfg("edos", 0, 0, n_hidden, n_atom_feats, n_bond_feats, 201, False, "")

    def _extra_dead(self, g):
        return super()._extra_dead(g) + _EDGE_ENCODER
