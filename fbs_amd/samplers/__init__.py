"""Mirror of fbs.samplers (fbs/samplers/__init__.py:1-3)."""
from .smc import (bootstrap_filter, filter_conditional_sampler, pmcmc_chain, pmcmc_kernel, sb_filter_conditional_sampler,
                  twisted_smc)
from .resampling import multinomial, systematic, stratified, killing
from .gibbs import gibbs_init, gibbs_kernel
from .gibbs_batched import gibbs_kernel_batched
from .smc_batched import (bootstrap_backward_smoother_batched, bootstrap_filter_batched, filter_key_schedule,
                          gibbs_init_batched, net_store_fits, pmcmc_filter_step_batched, pmcmc_kernel_batched,
                          pmcmc_key_schedule, smoother_key_schedule)
from .csmc.csmc import backward_sampling_pass_batched
from ..lg_kalman import kalman_conditional_sampler, kalman_path_sampler
from ..gaussian_sb import sb_kalman_conditional_sampler, sb_kalman_path_sampler
