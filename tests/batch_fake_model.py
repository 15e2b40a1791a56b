"""The attention-only fake model of tests/native_fake_model.py with a batch axis: the product's model contract for
``easykv_amd.generate_batch``.  One sequence (the prefill of each prompt, alone): ``position_ids [1, n]``, exactly the native model.
Several (the batched decode forward): ``position_ids [B', 1]``, each row its own position — row i takes rows ``pos[i]`` of the fixed
streams, so what a sequence sees does not depend on its neighbours — and ONE ``past_key_values.attend`` per layer with
``[B', heads, 1, D]``.  Logits are one-hot in each row's own position.  ``logs[s]`` collects, per sequence, the attention outputs of
every forward it took part in ``[layers, Hq, n, D]`` (a forward that starts at position 0 opens the next sequence's prefill)."""
from types import SimpleNamespace

import torch

from oracle.fake_model import FakeTokenizer, one_hot_logits


class BatchFakeModel:
    def __init__(self, qs, ks, vs, device="cuda", arch="LlamaForCausalLM", vocab=16):
        self.qs, self.ks, self.vs = qs.to(device).half(), ks.to(device).half(), vs.to(device).half()
        n_layers, hq, _, d = qs.shape
        self.config = SimpleNamespace(num_hidden_layers=n_layers, num_attention_heads=hq, num_key_value_heads=ks.shape[1],
                                      head_dim=d, architectures=[arch])
        self.device = torch.device(device)
        self.tokenizer = FakeTokenizer()
        self.vocab = vocab
        self.logs = []
        self.n_batched_forwards = 0

    def __call__(self, input_ids, past_key_values=None, position_ids=None, use_cache=True, **kw):
        b, n = position_ids.shape
        assert input_ids.shape == position_ids.shape and (b == 1 or n == 1)
        batched = hasattr(past_key_values, "live")
        outs = []
        for l in range(self.config.num_hidden_layers):
            # [heads, b, n, D] -> [b, heads, n, D]
            q, k, v = (t[l][:, position_ids].transpose(0, 1) for t in (self.qs, self.ks, self.vs))
            outs.append(past_key_values.attend(l, q, k, v))
        out = torch.stack(outs).float().cpu()      # [layers, b, Hq, n, D]
        if batched:
            self.n_batched_forwards += 1
            for row, s in enumerate(past_key_values.live):
                self.logs[s].append(out[:, row])
        else:
            if int(position_ids[0, 0]) == 0:
                self.logs.append([])
            self.logs[-1].append(out[:, 0])
        pos = position_ids.cpu()
        return SimpleNamespace(logits=torch.cat([one_hot_logits(pos[i], self.vocab) for i in range(b)]).to(self.device))
