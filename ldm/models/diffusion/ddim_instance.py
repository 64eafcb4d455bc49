from instancediffusion_amd.host.samplers import DDIMSamplerInst  # noqa: F401
