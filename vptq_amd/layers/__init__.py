from vptq_amd.layers.vqlinear import VQuantLinear, SiblingGroup, chain_prefetch, compact_model, link_siblings, prepare_model
from vptq_amd.layers.model_base import AutoModelForCausalLM

__all__ = ["VQuantLinear", "SiblingGroup", "chain_prefetch", "compact_model", "link_siblings", "prepare_model", "AutoModelForCausalLM"]
