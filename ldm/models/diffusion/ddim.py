from instancediffusion_amd.host.samplers import DDIMSampler  # noqa: F401
