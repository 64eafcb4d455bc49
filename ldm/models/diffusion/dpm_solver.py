from instancediffusion_amd.host.samplers import DPMSolverSampler, DPMSolverSamplerInst  # noqa: F401
