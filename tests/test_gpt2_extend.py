"""GPT2.extend and generate(prefill_chunk=...) on the CPU (fp32, the
reference path of `sdpa_kvcache`) against the plain forward."""

import pytest
import torch

from dmlcloud_amd.models.gpt2 import gpt2_tiny


@pytest.mark.parametrize('n_kv_head', [None, 1])
def test_extend_matches_the_plain_forward(n_kv_head):
    torch.manual_seed(0)
    model = gpt2_tiny(n_kv_head).eval()
    seq = torch.randint(0, 512, (2, 20))
    cache = model.init_cache(2, 20)
    end = 0
    with torch.no_grad():
        for chunk in (7, 1, 12):
            logits = model.extend(seq[:, end : end + chunk], cache)
            end += chunk
            torch.testing.assert_close(logits, model(seq[:, :end])[:, -1], rtol=0, atol=1e-4)
    assert cache.kv_len.tolist() == [20, 20]


def test_generate_with_prefill_chunk_gives_the_same_tokens():
    torch.manual_seed(0)
    model = gpt2_tiny().eval()
    prompt = torch.randint(0, 512, (2, 13))
    plain = model.generate(prompt, 6)
    assert plain.shape == (2, 19) and torch.equal(plain[:, :13], prompt)
    assert torch.equal(model.generate(prompt, 6, prefill_chunk=None), plain)
    assert torch.equal(model.generate(prompt, 6, prefill_chunk=5), plain)
